"""What the four yart_hip_scene_update* entries do with their `stats` argument, the same for each: a struct_size below the first two
fields is refused before the scene is looked at; otherwise struct_size is echoed, launches and the two times are written, and
exactly min(struct_size, sizeof(YartSceneUpdateStats)) bytes of the caller's memory are touched; NULL is taken. Through the binding's
raw library handle. On the device each entry runs the first step of the first case of its tests/test_*_update_host.py."""
import ctypes as C

import numpy as np
import pytest

FAKE = C.c_void_p(0x1000)                                     # a handle that is never dereferenced: the arguments are checked first
FILL, BUFFER = 0xA5, 40


def void(a):
    return a.ctypes.data_as(C.c_void_p)


def scene_args(api):
    """entry -> (its prefix, states -> (the update struct that takes a scene holding states[0] to states[1], what it points to))"""

    def transforms(s0, s1):
        nd = (api.NodeDesc * len(s1.nodes))(*[api.NodeDesc(n.parent, n.mesh, api._f(n.fwd, 16), api._f(n.inv, 16)) for n in s1.nodes])
        return api.SceneUpdate(C.sizeof(api.SceneUpdate), len(nd), nd, 0, None, 0), nd

    def meshes(s0, s1):
        changed = [m for m, (a, b) in enumerate(zip(s0.meshes, s1.meshes)) if not np.array_equal(a.positions, b.positions)]
        keep = [np.ascontiguousarray(s1.meshes[m].positions, np.float32) for m in changed]
        md = (api.MeshUpdate * len(changed))(*[api.MeshUpdate(m, len(p), void(p), None, None) for m, p in zip(changed, keep)])
        return api.SceneMeshUpdate(C.sizeof(api.SceneMeshUpdate), len(md), md, 0), (md, keep)

    def lighting(s0, s1):
        changed = [t for t, (a, b) in enumerate(zip(s0.textures, s1.textures)) if b.is_float and a.data.tobytes() != b.data.tobytes()]
        keep = [np.ascontiguousarray(s1.textures[t].data, np.float32) for t in changed]
        im = (api.EnvImageUpdate * len(changed))(*[api.EnvImageUpdate(t, p.shape[1], p.shape[0], void(p)) for t, p in zip(changed, keep)])
        return api.SceneLightingUpdate(C.sizeof(api.SceneLightingUpdate), 0, None, 0, None, len(im), im, 0), (im, keep)

    def textures(s0, s1):
        changed = [t for t, (a, b) in enumerate(zip(s0.textures, s1.textures)) if not b.is_float and a.data.tobytes() != b.data.tobytes()]
        keep = [np.ascontiguousarray(s1.textures[t].data, np.uint8) for t in changed]
        td = (api.TextureUpdate * len(changed))(*[api.TextureUpdate(t, s1.textures[t].width, s1.textures[t].height, s1.textures[t].channels,
                                                                    p.ctypes.data, 0) for t, p in zip(changed, keep)])
        return api.SceneTextureUpdate(C.sizeof(api.SceneTextureUpdate), len(td), td, 0), (td, keep)

    return {"yart_hip_scene_update": ("scene_update: ", transforms), "yart_hip_scene_update_meshes": ("scene_update_meshes: ", meshes),
            "yart_hip_scene_update_lighting": ("scene_update_lighting: ", lighting),
            "yart_hip_scene_update_textures": ("scene_update_textures: ", textures)}


ENTRIES = ["yart_hip_scene_update", "yart_hip_scene_update_meshes", "yart_hip_scene_update_lighting", "yart_hip_scene_update_textures"]


def first_states(entry):
    """the first state pair of the first case of the entry's host test"""
    if entry == "yart_hip_scene_update":
        from tests.test_scene_update_host import CASES, build_case
        return build_case(CASES[0])[:2]
    if entry == "yart_hip_scene_update_meshes":
        from tests.test_mesh_update_host import CASES, build_case
    elif entry == "yart_hip_scene_update_lighting":
        from tests.test_lighting_update_host import CASES, build_case
    else:
        from tests.test_texture_update_host import CASES, build_case
    return build_case(CASES[0])[0][:2]


@pytest.mark.parametrize("entry", ENTRIES)
def test_small_stats_are_refused_without_a_device(built, entry):
    """A well-formed update, a handle that is never dereferenced, stats.struct_size 0 and 4: YART_E_INVALID, `stats: struct_size` under
    the entry's prefix."""
    from yart_amd import api
    L = api.lib()
    prefix, make = scene_args(api)[entry]
    up, keep = make(*first_states(entry))
    for size in (0, 4):
        st = api.SceneUpdateStats(size)
        assert getattr(L, entry)(FAKE, C.byref(up), None, C.byref(st)) == api.YART_E_INVALID
        message = L.yart_hip_last_error().decode()
        assert message.startswith(prefix + "stats: struct_size"), message


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_stats_are_written_up_to_struct_size(built, entry):
    """struct_size 8, 16, 24 and 40 over 40 bytes of 0xA5: the call succeeds, struct_size reads back as given, launches are those the
    full struct reports for the same update, min(struct_size, 24) bytes are written and the bytes behind keep their 0xA5; NULL is
    taken. No frame is rendered."""
    from yart_amd import api
    L = api.lib()
    assert L.yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    s0, s1 = first_states(entry)
    up, keep = scene_args(api)[entry][1](s0, s1)
    scene = api.DeviceScene(s0, device=0)
    call = getattr(L, entry)
    full = api.SceneUpdateStats(C.sizeof(api.SceneUpdateStats))
    for _ in range(2):                                        # (the second call: the scene holds s1 already, as in every call below)
        api._check(call(scene._h, C.byref(up), None, C.byref(full)), L)
    assert full.struct_size == 24 and full.ms_total > 0 and full.ms_device >= 0
    for size in (8, 16, 24, 40):
        buf = (C.c_uint8 * BUFFER)(*[FILL] * BUFFER)
        C.c_uint32.from_buffer(buf).value = size
        api._check(call(scene._h, C.byref(up), None, C.cast(buf, C.POINTER(api.SceneUpdateStats))), L)
        got = api.SceneUpdateStats.from_buffer_copy(bytes(buf)[:24])
        print(entry, size, got.launches, got.ms_total, got.ms_device)
        assert got.struct_size == size and got.launches == full.launches
        written = min(size, 24)
        assert bytes(buf)[written:] == bytes([FILL]) * (BUFFER - written), "bytes behind the written part were touched"
        times = np.frombuffer(bytes(buf)[8:written], np.float64)
        assert np.isfinite(times).all() and (times >= 0).all() and (len(times) == 0 or times[0] > 0), "ms_total, ms_device were not written"
    api._check(call(scene._h, C.byref(up), None, None), L)
    scene.close()
