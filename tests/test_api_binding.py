"""The Python binding's shared pieces (yart_amd/api.py), without a device: the table of signatures against the header, the
builder of YartAovBuffers / YartMomentBuffers, the progressive-render runner against a Python stand-in for the C entry, and
_check's choice of library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

CAMERA = dict(size=(3, 2), eye=(0, 0, 3), target=(0, 0, 0), spp=8)


def declarations():
    """{export: [parameter, ...]} of include/yart_hip.h: comments removed (they hold commas, parentheses and the exports' names),
    then each ``yart_hip_name(`` up to its matching ``)``, split on the commas outside nested parentheses; ``(void)``: none."""
    text = open(os.path.join(ROOT, "include", "yart_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\b(yart_hip_[a-z0-9_]+)\s*\(", text):
        depth, params, cur = 1, [], ""
        for ch in text[m.end():]:
            depth += (ch == "(") - (ch == ")")
            if depth == 0:
                break
            if ch == "," and depth == 1:
                params.append(cur)
                cur = ""
            else:
                cur += ch
        params = [" ".join(s.split()) for s in params + [cur]]
        assert m.group(1) not in out, f"{m.group(1)} is declared twice"
        out[m.group(1)] = [] if params == ["void"] else params
    return out


def test_header_declarations_split_on_commas():
    """What the count below relies on: callbacks are typedefs, so no declaration nests parentheses, and no parameter is empty."""
    decl = declarations()
    assert len(decl) > 70
    for name, params in decl.items():
        for s in params:
            assert s and "(" not in s and ")" not in s, (name, s)
    assert decl["yart_hip_last_error"] == [] and len(decl["yart_hip_render"]) == 5 and len(decl["yart_hip_render_tiles"]) == 8


def test_signature_table_matches_header(built):
    from yart_amd import api
    decl = declarations()
    assert set(api.SIGNATURES) == set(api.EXPORTS) == set(decl)
    for name, (argtypes, restype) in api.SIGNATURES.items():
        assert len(argtypes) == len(decl[name]), (name, decl[name])
    returns = {n: r for n, (_, r) in api.SIGNATURES.items() if r is not C.c_int}
    assert returns == {"yart_hip_last_error": C.c_char_p, "yart_hip_scene_destroy": None, "yart_hip_multi_destroy": None,
                       "yart_hip_temporal_destroy": None, "yart_hip_exposure_destroy": None}
    L = api.lib()
    for name, (argtypes, restype) in api.SIGNATURES.items():
        fn = getattr(L, name)
        assert tuple(fn.argtypes) == tuple(argtypes) and fn.restype is restype, name
    assert len(L.yart_hip_multi_failed_devices.argtypes) == 3 and len(L.yart_hip_probe_shading.argtypes) == 5
    assert isinstance(L.yart_hip_last_error(), bytes)


@pytest.mark.parametrize("kind", ["aovs", "moments"])
def test_buffer_struct_host_forms(kind):
    from yart_amd import api
    cls, table = (api.AovBuffers, api.AOVS) if kind == "aovs" else (api.MomentBuffers, api.MOMENTS)
    h, w = 2, 3
    names = tuple(table)
    assert ("ids" in names and table["ids"][1:] == (4, np.int32)) or ("count" in names and table["count"][1:] == (1, np.uint32))

    def bits(ns):
        mask = 0
        for n in ns:
            mask |= table[n][0]
        return mask
    # allocated outputs
    for ask in (names, names[1:2], ()):
        st, bufs = api._buffer_struct(cls, table, h, w, ask)
        assert st.struct_size == C.sizeof(cls) and st.mask == bits(ask) and tuple(bufs) == tuple(ask)
        for n in names:
            if n not in ask:
                assert getattr(st, n) is None
                continue
            _, ch, dt = table[n]
            assert bufs[n].shape == ((h, w, ch) if ch > 1 else (h, w)) and bufs[n].dtype == dt and bufs[n].flags.c_contiguous
            assert getattr(st, n) == bufs[n].ctypes.data
    # host inputs: as they are where they fit, else contiguous copies in the table's dtype, kept alive by what is returned
    rng = np.random.default_rng(5)
    given = {}
    for i, n in enumerate(names):
        _, ch, dt = table[n]
        a = rng.integers(0, 100, (h, w, ch)).astype(dt)
        if i % 3 == 1:
            a = np.asfortranarray(np.concatenate([a, a], axis=1))[:, ::2]                  # not contiguous
        elif i % 3 == 2:
            a = a.astype(np.float64)                                                            # not the table's dtype
        given[n] = a
    st, kept = api._buffer_struct(cls, table, h, w, names, host=given)
    assert st.struct_size == C.sizeof(cls) and st.mask == bits(names)
    for n in names:
        _, ch, dt = table[n]
        assert kept[n].flags.c_contiguous and kept[n].dtype == dt and getattr(st, n) == kept[n].ctypes.data
        assert np.array_equal(kept[n].reshape(h, w, ch), given[n].astype(dt).reshape(h, w, ch))
    first = names[0]
    assert kept[first] is given[first]
    # names=None: every name of the mapping
    st, kept = api._buffer_struct(cls, table, h, w, host={names[-1]: given[names[-1]]})
    assert st.mask == bits(names[-1:]) and tuple(kept) == names[-1:]
    # a wrong size: the buffer's name
    for n in names:
        bad = dict(given, **{n: np.zeros((h, w + 1, table[n][1]), table[n][2])})
        with pytest.raises(AssertionError) as e:
            api._buffer_struct(cls, table, h, w, names, host=bad)
        assert str(e.value).splitlines()[0] == n
    # a missing name: KeyError where required, its bit clear where not (None counts as missing)
    fewer = {n: given[n] for n in names[1:]}
    with pytest.raises(KeyError):
        api._buffer_struct(cls, table, h, w, names, host=fewer)
    for partial in (fewer, dict(given, **{first: None})):
        st, kept = api._buffer_struct(cls, table, h, w, names, host=partial, required=False)
        assert st.mask == bits(names[1:]) and getattr(st, first) is None and first not in kept
    with pytest.raises(KeyError):
        api._buffer_struct(cls, table, h, w, ("no_such_buffer",))


def test_buffer_struct_keeps_the_callers_required_names():
    """pixel_motion's names are required, the temporal accumulator's are not"""
    from yart_amd import api
    aovs = {n: np.zeros((2, 3, api.AOVS[n][1]), api.AOVS[n][2]) for n in api.PIXEL_MOTION_AOVS if n != "ids"}
    with pytest.raises(KeyError):
        api._buffer_struct(api.AovBuffers, api.AOVS, 2, 3, api.PIXEL_MOTION_AOVS, host=aovs)
    st, _ = api._buffer_struct(api.AovBuffers, api.AOVS, 2, 3, api.TEMPORAL_AOVS, host=aovs, required=False)
    assert st.mask == api.AOVS["position"][0] | api.AOVS["normal"][0] | api.AOVS["coverage"][0]


class StandInLibrary:
    def __init__(self, message):
        self.message = message

    def yart_hip_last_error(self):
        return self.message


class StandInRender:
    """A Python stand-in for yart_hip_render_tiles / _waves: reports ``waves`` waves of ``tiles`` tiles each through the callbacks
    it is given, stops when one returns non-zero (YART_ABORTED), else returns ``rc``."""

    def __init__(self, tiles_arg, waves=2, tiles=2, rc=0, stats=True):
        self.tiles_arg, self.waves, self.tiles, self.rc, self.stats = tiles_arg, waves, tiles, rc, stats
        self.returned, self.null, self.calls = [], None, 0

    def __call__(self, handle, cam, params, frame, stats, *rest):
        from yart_amd import api
        self.calls += 1
        assert len(rest) == (3 if self.tiles_arg else 2) and rest[-1] is None
        on_wave, on_tile = rest[0], rest[1] if self.tiles_arg else None
        self.null = (not on_wave, not on_tile)
        assert isinstance(on_wave, api.WAVE_CALLBACK) and (on_tile is None or isinstance(on_tile, api.TILE_CALLBACK))
        wave_stats = api.Stats(rays=1234)
        for wave in range(self.waves):
            for k in range(self.tiles if on_tile else 0):
                tile = api.TileInfo(x=k, y=0, width=1, height=1, index=k + 1, total=self.tiles, wave=wave, rays=7)
                self.returned.append(("tile", on_tile(None, C.byref(tile))))           # a raise in on_tile must arrive here as 1
                if self.returned[-1][1]:
                    return 1
            if on_wave:
                self.returned.append(("wave", on_wave(None, C.addressof(wave_stats) if self.stats else None, wave, 4, 4 * (wave + 1), 8)))
                if self.returned[-1][1]:
                    return 1
        return self.rc


def run_progressive(fn, on_wave, on_tile=None, message=b"stand-in", **kw):
    from yart_amd import api
    return api._run_progressive(fn, StandInLibrary(message), None, CAMERA, on_wave, on_tile, **kw)


def test_progressive_runner_reports_and_stops():
    from yart_amd import api
    seen = []
    fn = StandInRender(True)
    frame, stats, aborted = run_progressive(fn, lambda f, info: seen.append((f, info)), lambda f, tile: seen.append((f, tile)))
    assert frame.shape == (2, 3, 4) and frame.dtype == np.float32 and not aborted and stats == api.Stats().asdict()
    assert fn.returned == [("tile", 0), ("tile", 0), ("wave", 0)] * 2 and fn.null == (False, False)
    assert all(f is frame for f, _ in seen)
    assert seen[2][1] == dict(wave=0, wave_samples=4, samples_taken=4, total_samples=8, rays=1234)
    assert seen[1][1] == api.TileInfo(x=1, y=0, width=1, height=1, index=2, total=2, wave=0, rays=7).asdict()
    # a true return: the trampoline returns 1, the stand-in returns YART_ABORTED, which is a result
    for stop_on in ("wave", "tile"):
        fn = StandInRender(True)
        out = run_progressive(fn, lambda f, info: stop_on == "wave" and "yes", lambda f, tile: stop_on == "tile" and tile["index"] == 2)
        assert out[2] is True and fn.returned[-1] == (stop_on, 1) and len(fn.returned) == (3 if stop_on == "wave" else 2)
    # the wave info carries rays exactly when asked for; a null stats pointer gives 0
    infos = []
    run_progressive(StandInRender(False), lambda f, info: infos.append(info), tiles=False, rays=False)
    assert infos[0] == dict(wave=0, wave_samples=4, samples_taken=4, total_samples=8)
    run_progressive(StandInRender(True, stats=False), lambda f, info: infos.append(info))
    assert infos[-1]["rays"] == 0
    # accumulated is copied into the frame
    acc = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    frame, _, _ = run_progressive(StandInRender(True), None, accumulated=acc)
    assert np.array_equal(frame, acc) and frame is not acc


def test_progressive_runner_null_callbacks():
    for tiles_arg in (True, False):
        fn = StandInRender(tiles_arg)
        out = run_progressive(fn, None, None, tiles=tiles_arg)
        assert fn.calls == 1 and fn.null == (True, True) and fn.returned == [] and out[2] is False
    fn = StandInRender(True)
    run_progressive(fn, None, lambda f, tile: None)
    assert fn.null == (True, False) and fn.returned == [("tile", 0)] * 4


@pytest.mark.parametrize("where", ["wave", "tile"])
def test_progressive_runner_carries_exceptions_past_the_c_frames(where):
    class Boom(Exception):
        pass

    def raiser(frame, info):
        raise Boom(where)
    quiet = lambda frame, info: None
    fn = StandInRender(True)
    with pytest.raises(Boom, match=where):
        run_progressive(fn, raiser if where == "wave" else quiet, raiser if where == "tile" else quiet)
    assert fn.calls == 1 and fn.returned[-1] == (where, 1)          # returned to the stand-in as 1, raised after it returned
    # KeyboardInterrupt and its like too
    def interrupt(frame, info):
        raise KeyboardInterrupt
    fn = StandInRender(True)
    with pytest.raises(KeyboardInterrupt):
        run_progressive(fn, interrupt, None)
    assert fn.returned == [("wave", 1)]


def test_progressive_runner_raises_the_librarys_error():
    from yart_amd import api
    with pytest.raises(api.YartError, match="from the stand-in") as e:
        run_progressive(StandInRender(True, rc=api.YART_E_HIP), None, message=b"from the stand-in")
    assert e.value.code == api.YART_E_HIP
    assert api.YART_ABORTED == 1
    assert run_progressive(StandInRender(True, rc=api.YART_ABORTED), None)[2] is True       # no error


class StandInTensor:
    """what _device_tensor asks of a torch tensor"""

    def __init__(self, shape, dtype="float32", itemsize=4, cuda=True, contiguous=True, ptr=0x7f0012345678):
        self.shape, self.dtype, self.itemsize, self.is_cuda, self.contiguous, self.ptr = shape, dtype, itemsize, cuda, contiguous, ptr

    def is_contiguous(self):
        return self.contiguous

    def numel(self):
        return int(np.prod(self.shape))

    def element_size(self):
        return self.itemsize

    def data_ptr(self):
        return self.ptr


def test_device_tensor_check_and_stream_default():
    from yart_amd import api
    t = StandInTensor((2, 3, 4))
    for ok in (dict(), dict(shape=(2, 3, 4)), dict(numel=24), dict(dtype="float32"), dict(element_size=4),
               dict(shape=[2, 3, 4], numel=24, dtype="float32", element_size=4)):
        p = api._device_tensor(t, "frame", **ok)
        assert isinstance(p, C.c_void_p) and p.value == t.ptr                          # the whole 64-bit pointer
    for bad in (dict(shape=(2, 3)), dict(numel=23), dict(dtype="int32"), dict(element_size=1)):
        with pytest.raises(AssertionError) as e:
            api._device_tensor(t, "frame", **bad)
        assert str(e.value) == "frame"
    for broken in (StandInTensor((2, 3, 4), cuda=False), StandInTensor((2, 3, 4), contiguous=False)):
        with pytest.raises(AssertionError):
            api._device_tensor(broken, "frame")
    assert api._device_tensor(None, "ldr", shape=(2, 3, 4), optional=True) is None
    with pytest.raises(AttributeError):
        api._device_tensor(None, "frame")
    # ids and counts travel as int32 tensors: the device form of the builder asks for the element size only
    ids = StandInTensor((2, 3, 4), dtype="int32", ptr=0x7f00aaaa0000)
    st, kept = api._buffer_struct(api.AovBuffers, api.AOVS, 2, 3, device={"ids": ids, "depth": StandInTensor((2, 3), ptr=64)})
    assert st.mask == api.AOVS["ids"][0] | api.AOVS["depth"][0] and st.ids == ids.ptr and st.depth == 64 and kept["ids"] is ids
    with pytest.raises(AssertionError) as e:
        api._buffer_struct(api.AovBuffers, api.AOVS, 2, 3, device={"depth": StandInTensor((2, 4))})
    assert str(e.value) == "depth"
    # an explicit stream is passed as it is, 0 / None without a tensor is the null stream
    assert api._stream_of(0x1234).value == 0x1234 and api._stream_of(0x1234, t).value == 0x1234
    assert api._stream_of(None) is None and api._stream_of(0) is None and api._stream_of(0, t) is None


def test_check_reports_the_library_that_was_called():
    from yart_amd import api
    plain, counting = StandInLibrary(b"the plain library's"), StandInLibrary(b"the instrumented library's")
    api._check(api.YART_OK, plain)
    for L in (plain, counting):
        with pytest.raises(api.YartError) as e:
            api._check(api.YART_E_INVALID, L)
        assert e.value.code == api.YART_E_INVALID and L.message.decode() in str(e.value)
    with pytest.raises(TypeError):
        api._check(api.YART_E_INVALID)
    with pytest.raises(TypeError):
        api._check(api.YART_OK)
