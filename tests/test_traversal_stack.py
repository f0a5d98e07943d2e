"""The lane-private traversal stack at every depth boundary (csrc/traverse.hpp: TravStack, stackPush / Pop / Peek / Poke).

A ray's stack lives in two places: the first entries in LDS (8 for the lean kernels, 16 for the general wavefront kernels, 24
for the megakernel, the probe and the feature-buffer kernels), the rest in a lane-interleaved spill area; a lean walk hands
its ray over WITH its stack when it holds at most 16 entries (resume record) and restarts it otherwise. The spill area is
sized at scene creation from the scene's stack bound (csrc/host_scene.hpp), and a mesh whose tree needs more than
kMaxStackBound = 192 entries is refused there.

scenes.deep_tree(levels) builds a mesh whose BVH is a chain of exactly `levels` inner nodes which the central rays descend
with both children hit at every level. `hostsim stackcheck` measures what the rays of a frame reach — a case counts only if
the histogram has rays at the depth it is named after. CPU: the device headers compiled for the host with a REAL split
(`split` entries in one heap block, the rest in another of exactly the bound's size, lane-interleaved with stride > 1) under
AddressSanitizer + UBSan, against the compiled reference. GPU: every pipeline, every lean form, the feature buffers.

Finite f32 geometry drives the reference's builder to about 80 levels (scenes.chain_mesh), not past the cap of 192: the
refusal is tested on a synthetic node array through the functions scene creation calls (`hostsim stackbound`)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ORACLE_BIN, REF_BIN, ROOT

LEVELS = [7, 8, 9, 15, 16, 17, 23, 24, 25, 40, 63, 64]
SPLITS = [8, 16, 24, 64]            # lean kernels, general wavefront kernels, megakernel / probe / AOV kernels, no spill at all
ALPHA = (3, 8, 9, 16, 17, 24, 25)   # stack entries a walk holds when it tests an alpha-tested triangle
OVER = 70                           # more than the reference's 64, within the cap
GUARD_TEXT = b"the traversal stack holds at most"       # host_scene.hpp::checkStackBound, compiled into the library


def _checker():
    exe = REF_BIN if os.path.exists(REF_BIN) else ORACLE_BIN
    if not os.path.exists(exe):
        pytest.skip("neither oracle/_ref/yart_ref nor the oracle restatement is built")
    return exe


def _case(tmp_path, levels, instances=0, tag="s", **kw):
    from yart_amd import scenes
    kw.setdefault("spp", 2)
    s, p = scenes.deep_tree(levels, alpha_levels=tuple(a for a in ALPHA if a < levels), instances=instances, **kw)
    sp, pp = str(tmp_path / f"{tag}.yscn"), str(tmp_path / f"{tag}.txt")
    s.save(sp); scenes.write_params(pp, p)
    return s, p, sp, pp


def _stackcheck(exe, sp, pp, out, env=None):
    r = subprocess.run([exe, "stackcheck", sp, pp, out], check=True, capture_output=True, text=True, env=env)
    return json.loads(r.stdout.strip().splitlines()[-1])


def _reference(sp, pp, out):
    r = subprocess.run([_checker(), "render", sp, pp, out], check=True, capture_output=True, text=True)
    return int(json.loads(r.stdout.strip().splitlines()[-1])["rays"])


@pytest.fixture(scope="module")
def stack_san(built):
    """tests/hostsim with -fsanitize=address,undefined: the binary of tests/test_sanitizers.py, built by whichever module
    needs it first and rebuilt when a source is newer."""
    from tests.test_sanitizers import SAN, SRC
    newest = max(os.path.getmtime(os.path.join(dp, f)) for d in ("yart_amd/csrc", "tests/hostsim", "oracle")
                 for dp, _, fs in os.walk(os.path.join(ROOT, d)) for f in fs if f.endswith((".hpp", ".cpp", ".inc")))
    if not os.path.exists(SAN) or os.path.getmtime(SAN) < newest:
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-ffp-contract=off", "-o", SAN] + SRC + ["-lpthread"], capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("no sanitizer runtime for g++ here: " + r.stderr[-200:])
    return SAN


def _san_render(san, sp, pp, out, split, bound=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", YART_HOSTSIM_LDS_STACK=str(split))
    if bound is not None:
        env["YART_HOSTSIM_STACK_BOUND"] = str(bound)
    return subprocess.run([san, "render", sp, pp, out], capture_output=True, text=True, env=env)


def _clean(r):
    return r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _nonzero(h):
    return {k: v for k, v in enumerate(h) if v}


@pytest.mark.parametrize("levels", LEVELS)
def test_generator_reaches_exactly_the_depth(hostsim, hostsim_lean, tmp_path, levels):
    """The chain mesh's tree needs exactly `levels` entries, rays of the frame hold exactly that many (and every smaller
    number), none holds more; the fast walk's hand-overs fall on both sides of the lean kernels' LDS seam (8 | 9) and of the
    resume record's capacity (16 | 17) wherever the tree is deep enough for that."""
    _, _, sp, pp = _case(tmp_path, levels)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    hist = info["ray_max_hist"]
    print(f"levels {levels}: need {info['mesh_need']} bound {info['stack_bound']} max {info['max_stack_index']} rays per maximum {_nonzero(hist)}")
    assert max(info["mesh_need"]) == levels and info["stack_bound"] == levels
    assert info["max_stack_index"] == levels, "no ray may hold more entries than the tree has inner levels, one must hold all"
    assert hist[levels] >= 100, "the frame must have rays at the depth the case is named after"
    assert all(hist[k] > 0 for k in range(levels + 1)), "every depth below it is reached as well"
    assert sum(hist[levels + 1:]) == 0
    lean = _stackcheck(hostsim_lean, sp, pp, str(tmp_path / "l.f32"))
    hand = lean["handover_hist"]
    print(f"levels {levels}: hand-overs per stack entries held {_nonzero(hand)}")
    assert sum(hand[levels + 1:]) == 0
    assert sum(hand) > 0
    for lo, hi in ((8, 9), (16, 17)):
        if levels > hi:
            assert hand[lo] > 0 and hand[hi] > 0, f"hand-overs with exactly {lo} and {hi} entries"
            assert sum(hand[:lo + 1]) > 0 and sum(hand[hi:]) > 0
    # the fast walk keeps or hands over; either way the frame is the general walk's
    assert np.array_equal(np.fromfile(tmp_path / "g.f32", np.uint32), np.fromfile(tmp_path / "l.f32", np.uint32))


@pytest.mark.parametrize("levels", LEVELS)
def test_split_stack_is_the_reference_frame(stack_san, tmp_path, levels):
    """Each split of the stack (8 / 16 / 24 entries in the first block, the rest in a spill block of exactly the remaining
    size, lane-interleaved) renders the reference's frame word for word, and the sanitizers report nothing."""
    _, _, sp, pp = _case(tmp_path, levels)
    ref = str(tmp_path / "ref.f32")
    _reference(sp, pp, ref)
    want = np.fromfile(ref, np.uint32)
    for split in SPLITS:
        out = str(tmp_path / f"san{split}.f32")
        r = _san_render(stack_san, sp, pp, out, split)
        assert _clean(r), (split, r.stderr[-1500:])
        got = np.fromfile(out, np.uint32)
        assert np.array_equal(want, got), f"split {split}: {(want != got).sum()} words differ"


def test_stack_primitives_at_every_split(stack_san):
    """stackPush / Pop / Peek / Poke on three interleaved lanes, every split from 1 to the bound, bounds 64 and 70: each entry
    comes back as written, to its own lane, from whichever block holds it (stackPeek and stackPoke are what the resume
    records of the lean kernels go through: only the device calls them otherwise); nothing is touched outside the blocks."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for bound in (64, OVER):
        r = subprocess.run([stack_san, "stackops", "0", str(bound)], capture_output=True, text=True, env=env)
        assert _clean(r) and len(r.stdout.splitlines()) == bound, (bound, r.stderr[-1200:])


def test_instanced_chain_on_host(stack_san, hostsim, tmp_path):
    """The chain under rotated, non-uniformly scaled nodes (the general walk): same depths, same frame as the reference."""
    _, _, sp, pp = _case(tmp_path, 25, instances=5)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert info["max_stack_index"] == 25 and info["ray_max_hist"][25] > 0 and info["ray_max_hist"][24] > 0
    ref = str(tmp_path / "ref.f32")
    _reference(sp, pp, ref)
    for split in (8, 24):
        out = str(tmp_path / "san.f32")
        r = _san_render(stack_san, sp, pp, out, split)
        assert _clean(r), r.stderr[-1500:]
        assert np.array_equal(np.fromfile(ref, np.uint32), np.fromfile(out, np.uint32)), split


@pytest.mark.parametrize("levels", [25, 64])
def test_chain_known_answers(hostsim, tmp_path, levels):
    """Hit records and per-sample radiance of probe rays down the chain: every vector equals the compiled reference's."""
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/yart_ref is not built")
    from yart_amd import scenes
    from tests import katlib
    s, p, sp, pp = _case(tmp_path, levels)
    rng = np.random.RandomState(levels)
    probes = [(int(rng.randint(16, 32)), int(rng.randint(16, 32))) for _ in range(8)]
    scenes.write_params(pp, p, threads=1, probe_pixels=probes)
    kats = {}
    for name, exe in (("ref", REF_BIN), ("device", hostsim)):
        out = str(tmp_path / (name + ".json"))
        subprocess.run([exe, "kat", sp, pp, out], check=True, stdout=subprocess.DEVNULL)
        kats[name] = katlib.load(out)
    res = katlib.compare(kats["ref"], kats["device"], [k for k in kats["ref"] if k != "ggxGlassEavg"])
    bad = {k: v for k, v in res.items() if v["mismatches"]}
    assert not bad, bad


def test_more_than_64_entries_on_host(stack_san, hostsim, tmp_path):
    """A tree of 70 levels: with the spill block sized from the scene's bound every split renders without a report and all
    splits agree; with the block as it used to be — 64 entries whatever the scene — AddressSanitizer reports the write
    past it (so would one entry short of the bound). The reference's own stack has 64 entries and its behaviour here is
    undefined: what it does is printed, not asserted."""
    _, _, sp, pp = _case(tmp_path, OVER)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert max(info["mesh_need"]) == OVER and info["stack_bound"] == OVER and info["max_stack_index"] == OVER
    assert info["ray_max_hist"][64] >= 100            # (the last bin: 64 entries and more)
    frames = []
    for split in SPLITS:
        out = str(tmp_path / f"san{split}.f32")
        r = _san_render(stack_san, sp, pp, out, split)
        assert _clean(r), (split, r.stderr[-1500:])
        frames.append(np.fromfile(out, np.uint32))
        assert np.array_equal(frames[0], frames[-1]), split
    assert np.array_equal(frames[0], np.fromfile(tmp_path / "g.f32", np.uint32))
    for bound in (64, OVER - 1):
        r = _san_render(stack_san, sp, pp, str(tmp_path / "short.f32"), 8, bound=bound)
        assert r.returncode != 0 and "heap-buffer-overflow" in r.stderr and "stackPush" in r.stderr, (bound, r.stderr[-800:])
    ref = str(tmp_path / "ref.f32")
    r = subprocess.run([_checker(), "render", sp, pp, ref], capture_output=True, text=True)       # (a child process: it may crash)
    if r.returncode != 0 or not os.path.exists(ref):
        print(f"the reference does not survive {OVER} levels: exit status {r.returncode}")
    else:
        print(f"the reference survives {OVER} levels; words differing from the device headers' frame: "
              f"{int((np.fromfile(ref, np.uint32) != frames[0]).sum())}")


def test_scene_creation_refuses_past_the_cap(hostsim):
    """bvhStackNeed + checkStackBound (what buildHostImage runs on every mesh) on chains of inner nodes: the need is the
    number of inner levels, exactly; 192 passes, 193 and 5000 (no recursion) are refused with a message that names the mesh
    and its depth. The check sits behind hipSetDevice in yart_hip_scene_create, hence here at the host_scene.hpp level."""
    for levels, refused in ((0, False), (1, False), (64, False), (65, False), (192, False), (193, True), (5000, True)):
        info = json.loads(subprocess.run([hostsim, "stackbound", str(levels)], check=True, capture_output=True, text=True).stdout)
        assert info["need"] == levels and info["cap"] == 192 and info["refused"] is refused, info
        if refused:
            assert "mesh 0" in info["message"] and str(levels) in info["message"] and "192" in info["message"], info


def test_unchanged_scenes_keep_their_bound(hostsim, tmp_path):
    """The goldens stay far below 64 (their spill areas are sized as before); a scene of 70 nodes reports the height of its
    top-level hierarchy, which a median split keeps logarithmic."""
    from yart_amd import scenes
    base = os.path.join(ROOT, "tests", "golden", "cornell")
    info = _stackcheck(hostsim, base + ".yscn", base + ".txt", str(tmp_path / "c.f32"))
    assert 0 < info["stack_bound"] < 64 and info["tlas_height"] == 0 and info["max_stack_index"] <= info["stack_bound"]
    s, p = scenes.instances(24, 24, 1, 2, n_instances=70)
    sp, pp = str(tmp_path / "i.yscn"), str(tmp_path / "i.txt")
    s.save(sp); scenes.write_params(pp, p)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "i.f32"))
    assert info["tlas_height"] == 7, info["tlas_height"]            # 71 mesh nodes: ceil(log2 71)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def _every_pipeline(api, s, p, ref_path, ref_rays, tag):
    from tests.test_gpu_parity import PIPELINE_FLAGS
    scene = api.DeviceScene(s, device=0)
    want = None
    try:
        for name, flags in PIPELINE_FLAGS.items():
            img, st = scene.render(p, flags=flags)
            if want is None:
                want = np.fromfile(ref_path, np.float32).reshape(img.shape)
            diff = int((img.view(np.uint32) != want.view(np.uint32)).sum())
            print(f"{tag} / {name}: words differing {diff}, rays {st['rays']} (reference {ref_rays})")
            assert np.array_equal(img.view(np.uint32), want.view(np.uint32)), f"{tag} / {name}: {diff} words differ"
            assert int(st["rays"]) == ref_rays, f"{tag} / {name}: {st['rays']} rays, the reference counts {ref_rays}"
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", LEVELS)
def test_chain_on_device(gpu_api, ref_bin, hostsim, tmp_path, levels):
    """Every pipeline — the lean kernels with resume records and with restarts, the general kernels, the megakernel — on rays
    that hold exactly `levels` entries: the compiled reference's frame on every word, and its ray count."""
    s, p, sp, pp = _case(tmp_path, levels)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert info["max_stack_index"] == levels and info["ray_max_hist"][levels] >= 100
    ref = str(tmp_path / "ref.f32")
    rays = _reference(sp, pp, ref)
    _every_pipeline(gpu_api, s, p, ref, rays, f"chain of {levels}")


@pytest.mark.gpu
@pytest.mark.parametrize("instances", [5, 30, 70])
def test_instanced_chain_on_device(gpu_api, ref_bin, hostsim, tmp_path, instances):
    """The chain under rotated, non-uniformly scaled nodes: the general (non-identity) walk through the same seams. 5
    instances: the scene tables in LDS; 30: one candidate mask; 70 (more than 64 nodes): the top-level hierarchy by default,
    chunked masks and the per-lane node walk through their pipeline flags."""
    s, p, sp, pp = _case(tmp_path, 25, instances=instances)
    assert (len(s.nodes) <= 16) == (instances == 5) and (len(s.nodes) >= 64) == (instances == 70)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert info["max_stack_index"] == 25 and all(info["ray_max_hist"][k] > 0 for k in (8, 9, 16, 17, 24, 25))
    ref = str(tmp_path / "ref.f32")
    rays = _reference(sp, pp, ref)
    _every_pipeline(gpu_api, s, p, ref, rays, f"{instances} instances of a chain of 25")


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [24, 25, 64])
def test_chain_feature_buffers_vs_host_walk(gpu_api, hostsim, tmp_path, levels):
    """The probe / feature-buffer kernels keep 24 entries in LDS: depth, ids and the other buffers of the chain scene equal
    the host walk's (tests/aovsim) on every pixel."""
    from tests import test_aovs
    exe = str(tmp_path / "aovsim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "aovsim", "aovsim.cpp"),
                    os.path.join(ROOT, "yart_amd", "csrc", "_gen", "lut_data.cpp"), "-lpthread"], check=True)
    s, p, sp, pp = _case(tmp_path, levels)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert info["max_stack_index"] == levels and info["ray_max_hist"][levels] >= 100
    w, h = p["size"]
    spp = p["spp"]
    host = test_aovs._host_hits(exe, tmp_path, sp, pp, test_aovs._triples(w, h, spp))
    exp = test_aovs._expected(gpu_api, host, h, w, spp)
    scene = gpu_api.DeviceScene(s, device=0)
    try:
        frame, got, st = scene.render_aovs(p)
        plain, st0 = scene.render(p)
    finally:
        scene.close()
    for name in ("depth", "normal", "position", "coverage", "albedo"):
        test_aovs.same_bits(got[name], exp[name], f"chain of {levels}: {name} vs host walk")
    assert np.array_equal(got["ids"], exp["ids"]), "ids"
    assert (got["ids"][..., 1] == 1).sum() > 100, "the chain mesh must be what many pixels see first"
    test_aovs.same_bits(frame, plain, "frame of render_aovs vs render")
    assert st["rays"] == st0["rays"]


@pytest.mark.gpu
def test_more_than_64_entries_on_device(gpu_api, stack_san, hostsim, tmp_path):
    """A tree of 70 levels renders in every pipeline and equals the host sanitizer build's frame. Before anything is
    launched: the scene's bound is what the test expects, and the library is one compiled with the bound (the refusal text of
    host_scene.hpp is in it) — a library that sizes the spill area for 64 entries whatever the scene is not given this scene."""
    s, p, sp, pp = _case(tmp_path, OVER)
    info = _stackcheck(hostsim, sp, pp, str(tmp_path / "g.f32"))
    assert info["stack_bound"] == OVER and info["max_stack_index"] == OVER and info["spill_entries"] == 0 and info["lds_entries"] == OVER
    with open(os.path.join(ROOT, "yart_amd", "libyart_hip.so"), "rb") as f:
        assert GUARD_TEXT in f.read(), "libyart_hip.so has no stack bound: not rendering a scene that needs more than 64 entries"
    out = str(tmp_path / "san.f32")
    r = _san_render(stack_san, sp, pp, out, 8)
    assert _clean(r), r.stderr[-1500:]
    rays = int(json.loads(r.stdout.strip().splitlines()[-1])["rays"])
    _every_pipeline(gpu_api, s, p, out, rays, f"chain of {OVER}")
