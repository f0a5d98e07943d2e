"""The scene walk per ray, at the places where a traversal goes wrong (tests/raysuite.py): box planes and NaN slab terms,
shared edges and vertices, equal distances, the determinant's epsilon, instance culls, alpha-tested and transparent cards.

The committed records (tests/golden/rays/<suite>.rec) are the compiled reference's own testNode per ray (`yart_ref hits`,
oracle/rayrec.hpp). On the CPU the oracle restatement, the host build of the device headers (hostsim, hostsim_lean) and — where
it is built — the live reference must give them bit for bit, and the suites must meet the events they are aimed at (the oracle
counts them per ray). On the GPU every instantiation of traverseScene (yart_hip_probe_rays: general, fast, fast + identity; both
ray kinds) is compared with the same records."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import raysuite
from tests.conftest import GOLDEN, REF_BIN, ROOT
from tests.paramfile import load_params

RAYS = os.path.join(GOLDEN, "rays")
LARGEST_FIXTURE = 294348          # tests/golden/material.yscn


def base(suite):
    return os.path.join(RAYS, suite)


def committed(suite):
    rays = np.fromfile(base(suite) + ".rays", raysuite.RAY)
    rec = np.fromfile(base(suite) + ".rec", raysuite.REC)
    ev = np.fromfile(base(suite) + ".events", np.uint16)
    assert len(rays) == len(rec) == len(ev) > 0
    return rays, rec, ev


def run_hits(exe, suite, out, *extra):
    return subprocess.run([exe, "hits", base(suite) + ".yscn", base(suite) + ".txt", base(suite) + ".rays", str(out), *extra],
                          check=True, capture_output=True, text=True)


def same_records(got, want, what):
    assert len(got) == len(want), what
    g, w = got.view(np.uint32).reshape(len(got), -1), want.view(np.uint32).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(g)} records differ, first ray {bad[0]}: got {got[bad[0]]}, committed {want[bad[0]]}"


@pytest.fixture(scope="session")
def live_reference():
    """oracle/_ref/yart_ref where it is built and has the `hits` mode (its usage line names it), else None. A binary carried
    over from a tree that had no such mode is rebuilt first where the reference's sources are (oracle/Makefile rebuilds the
    driver when its sources' content changed); without the sources the committed records, which are that reference's own,
    stand alone."""
    def has_hits():
        return os.path.exists(REF_BIN) and " hits " in subprocess.run([REF_BIN], capture_output=True, text=True).stderr
    if os.path.exists(REF_BIN) and not has_hits():
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], capture_output=True)
    return REF_BIN if has_hits() else None


# ------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_generator_reproduces_the_fixtures(suite, tmp_path):
    from yart_amd import scenes
    s, p, rays = raysuite.build(suite)
    assert s.tobytes() == open(base(suite) + ".yscn", "rb").read(), "scene"
    assert rays.tobytes() == open(base(suite) + ".rays", "rb").read(), "rays"
    scenes.write_params(tmp_path / "p.txt", p)
    assert open(tmp_path / "p.txt").read() == open(base(suite) + ".txt").read(), "params"
    assert s.n_triangles <= 5000 and len(rays) <= raysuite.MAX_RAYS
    assert np.isfinite(rays["o"]).all() and np.isfinite(rays["d"]).all()
    for ext in (".yscn", ".txt", ".rays", ".rec", ".events", ".events.json"):
        assert os.path.getsize(base(suite) + ext) <= LARGEST_FIXTURE, ext


def test_all_suites_hold_at_most_100000_rays():
    assert sum(os.path.getsize(base(s) + ".rays") // raysuite.RAY.itemsize for s in raysuite.SUITES) <= 100000


@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_oracle_and_reference_give_the_committed_records(suite, oracle_bin, live_reference, tmp_path):
    """The oracle restatement — and the compiled reference itself where it is built — against the committed records, and the
    oracle's event masks and counts against the committed ones."""
    _, rec, ev = committed(suite)
    r = run_hits(oracle_bin, suite, tmp_path / "o.rec")
    same_records(np.fromfile(tmp_path / "o.rec", raysuite.REC), rec, f"{suite}: oracle")
    assert np.array_equal(np.fromfile(str(tmp_path / "o.rec") + ".events", np.uint16), ev), "event masks"
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.load(open(base(suite) + ".events.json")), "event counts"
    if live_reference:
        run_hits(live_reference, suite, tmp_path / "r.rec")
        same_records(np.fromfile(tmp_path / "r.rec", raysuite.REC), rec, f"{suite}: compiled reference")


@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_hostsim_gives_the_committed_records(suite, hostsim, tmp_path):
    """csrc/traverse.hpp compiled for the host: traverseScene<false / true> + finalizeHit, bit for bit."""
    _, rec, _ = committed(suite)
    run_hits(hostsim, suite, tmp_path / "h.rec")
    same_records(np.fromfile(tmp_path / "h.rec", raysuite.REC), rec, f"{suite}: hostsim")


@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_hostsim_lean_keeps_no_ray_that_differs(suite, hostsim_lean, tmp_path):
    """The hand-over build: the records are the general walk's, and no ray the TRAV_FAST walks keep differs from it."""
    _, rec, _ = committed(suite)
    r = run_hits(hostsim_lean, suite, tmp_path / "l.rec")
    same_records(np.fromfile(tmp_path / "l.rec", raysuite.REC), rec, f"{suite}: hostsim_lean")
    assert "differs" not in r.stderr, r.stderr[:2000]
    assert json.loads(r.stdout.strip().splitlines()[-1])["kept_rays_that_differ"] == 0


@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_event_floors(suite):
    """A suite meets the events it is aimed at: at least 64 rays each, at least 8 for t == tMin and t == tMax. A condition on the
    rays, not a measurement: rays that miss a floor are changed, the floor is not."""
    _, _, ev = committed(suite)
    counts = json.load(open(base(suite) + ".events.json"))
    for k, name in enumerate(raysuite.EVENTS):
        assert int(((ev >> k) & 1).sum()) == counts[name], name
    print(suite, counts)
    for name in raysuite.TARGETS[suite]:
        floor = raysuite.FLOOR_T if name in ("t_eq_tmin", "t_eq_tmax") else raysuite.FLOOR
        assert counts[name] >= floor, f"{suite}: {counts[name]} rays meet {name}, the floor is {floor}"


def test_every_event_is_some_suites_target():
    assert sorted(e for t in raysuite.TARGETS.values() for e in t) == sorted(raysuite.EVENTS)


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def is_identity_scene(path):
    from yart_amd.yscn import Scene
    eye = np.eye(4, dtype=np.float32)
    return all(np.array_equal(n.fwd, eye) and np.array_equal(n.inv, eye) for n in Scene.load(path).nodes)


def has_alpha_or_transparent(path):
    from yart_amd.yscn import Scene
    s = Scene.load(path)
    return any(m.tex_base >= 0 or (m.thin_transmission and m.transmission > 0.0) for m in s.materials)


@pytest.mark.gpu
@pytest.mark.parametrize("suite", raysuite.SUITES)
def test_device_walks_vs_committed_records(api, suite):
    """One DeviceScene per suite, reading tests/golden only. Walk 0 (TRAV_GENERAL) gives the committed records bit for bit, both
    kinds. Walks 1 (TRAV_FAST) and, on identity scenes, 2 (TRAV_FAST | TRAV_IDENTITY): a ray that is not handed over gives the
    committed record (an occlusion ray: the flag, the attenuation of an unoccluded ray and the draw — all a fast occlusion walk
    reports); every closest-hit ray with an alpha-tested candidate is handed over (a transparent surface is an ordinary hit for a
    closest-hit ray, traverse.hpp: such a ray is kept and its record is the committed one), and an occlusion ray that is kept and
    ends unoccluded met neither kind of candidate; no ray is handed over in a suite without such materials.
    yart_hip_probe_hits still equals walk 0 on the closest-hit rays."""
    rays, rec, ev = committed(suite)
    p = load_params(base(suite) + ".txt")
    scene = api.DeviceScene(base(suite) + ".yscn", device=0)
    try:
        got = scene.probe_rays(p, rays, 0).view(raysuite.REC).reshape(-1)
        same_records(got, rec, f"{suite}: walk 0")
        closest = rays["kind"] == 0
        alpha = (ev & raysuite.ALPHA_BIT) != 0
        transparent = (ev & raysuite.TRANSPARENT_BIT) != 0
        walks = [1, 2] if is_identity_scene(base(suite) + ".yscn") else [1]
        for walk in walks:
            fast = scene.probe_rays(p, rays, walk).view(raysuite.REC).reshape(-1)
            deferred = fast["deferred"] != 0
            assert set(np.unique(fast["deferred"])) <= {0, 1}
            keep = ~deferred
            assert keep.any()
            same_records(fast[keep & closest], rec[keep & closest], f"{suite}: walk {walk}, closest-hit rays it keeps")
            occ = keep & ~closest
            assert np.array_equal(fast["hit"][occ], rec["hit"][occ]), f"{suite}: walk {walk}, occluded"
            assert np.array_equal(fast["draw"][occ].view(np.uint32), rec["draw"][occ].view(np.uint32)), f"{suite}: walk {walk}, draw"
            free = occ & (rec["hit"] == 0)
            assert np.array_equal(fast["att"][free].view(np.uint32), rec["att"][free].view(np.uint32)), f"{suite}: walk {walk}, attenuation"
            assert deferred[closest & alpha].all(), f"{suite}: walk {walk} kept a closest-hit ray with an alpha-tested candidate"
            assert not (alpha | transparent)[free].any(), f"{suite}: walk {walk} kept an unoccluded ray that met an alpha / transparent candidate"
            assert not fast[deferred].view(np.uint32).reshape(-1, 20)[:, :18].any(), "a handed-over record is zero but for its flag"
            if not has_alpha_or_transparent(base(suite) + ".yscn"):
                assert not alpha.any() and not transparent.any() and not deferred.any(), f"{suite}: walk {walk} handed over {int(deferred.sum())} rays"
            else:
                assert deferred.any()
        # probe_hits: the same walk with tMax = inf and a sampler of its own (so only rays without alpha draws compare)
        plain = closest & np.isposinf(rays["tmax"]) & ~alpha
        assert plain.any()
        six = np.concatenate([rays["o"][plain], rays["d"][plain]], axis=1)
        ph = scene.probe_hits(six)
        g = got[plain]
        assert np.array_equal(ph[:, 0] > 0.5, g["hit"] != 0)
        hit = g["hit"] != 0
        a = np.ascontiguousarray(np.concatenate([ph[hit, 1:2], ph[hit, 4:13]], axis=1))
        b = np.ascontiguousarray(np.concatenate([g["t"][hit, None], g["p"][hit], g["n"][hit], g["tg"][hit]], axis=1))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "probe_hits: t, p, n, tangent"
        assert np.array_equal(ph[hit, 13].astype(np.int64), g["tri"][hit].astype(np.int64))
        assert np.array_equal(ph[hit, 14].astype(np.int64), g["light"][hit].astype(np.int64))
        assert np.array_equal(ph[hit, 15].astype(np.int64), g["back"][hit].astype(np.int64))
    finally:
        scene.close()


@pytest.mark.gpu
def test_probe_rays_refusals(api):
    import ctypes as C
    L = api.lib()
    rays, _, _ = committed("instances")
    p = load_params(base("instances") + ".txt")
    rp = api.make_params(p)
    one = np.ascontiguousarray(rays[:1])
    out = np.zeros(20, np.uint32)
    ptr, optr = one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    scene = api.DeviceScene(base("instances") + ".yscn", device=0)
    try:
        h = scene._h
        assert L.yart_hip_probe_rays(None, C.byref(rp), 1, ptr, 0, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_rays(h, None, 1, ptr, 0, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, None, 0, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, ptr, 0, None) == api.YART_E_INVALID
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, ptr, 3, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, ptr, 2, optr) == api.YART_E_INVALID, "walk 2 on a transformed scene"
        for field, value in (("x", 65536), ("y", 65536), ("s", int(p["spp"])), ("kind", 2)):
            bad = one.copy()
            bad[field] = value
            assert L.yart_hip_probe_rays(h, C.byref(rp), 1, bad.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID, field
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, ptr, 0, optr) == 0
        assert L.yart_hip_probe_rays(h, C.byref(rp), 1, ptr, 1, optr) == 0
    finally:
        scene.close()
