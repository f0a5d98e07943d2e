"""The shading code per call, at the places where it goes wrong (tests/shadesuite.py): texture fetches at the last texel column and
at fractional weights of exactly 0, GGX table lookups on the tables' lattices and at the index caps, every lobe and mixture of the
parametric BSDF with uc2 one float either side of its thresholds, lights sampled exactly on CDF entries and guide brackets, the
light pick at the boundary between the infinite and the area lights.

The committed records (tests/golden/shading/<suite>.rec) are the compiled reference's own Texture / LUT functions / BSDF / Light /
PowerLightSampler per case (`yart_ref shade`, oracle/shaderec.hpp). On the CPU the oracle restatement, the host build of the device
headers (hostsim, through the plain entries and through matEvaluate + the *ImplE entries) and — where it is built — the live
reference must give them, and the suites must meet the events they are aimed at (the oracle reports them per case). On the GPU
yart_hip_probe_shading is compared with the same records in every form only the device runs: the GGX tables in LDS, the scene's
record tables in LDS, the *ImplE entries, with and without 2x2 footprint records of the textures.

Every result is compared on bits, with one exception: a word that is NaN in the committed record must be NaN in the result, sign
and payload ignored (x86 and the GPU propagate payloads differently). Fewer than 1 % of a suite's result words are NaN."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import shadesuite
from tests.conftest import GOLDEN, REF_BIN, ROOT

SHADING = os.path.join(GOLDEN, "shading")
LARGEST_FIXTURE = 294348          # tests/golden/material.yscn
FORMS = [0, 1, 2, 4, 7]
BUNDLE_TEXTURES = [12, 13, 14]     # shadesuite.textures(): base colour, normal and metal-rough maps of the bundled material
KAT_GOLDENS = ["cornell", "material", "cornell_waves", "uniform_sky", "two_skies"]


def base(suite):
    return os.path.join(SHADING, suite)


def committed(suite):
    cases = np.fromfile(base(suite) + ".cases", shadesuite.CASE)
    rec = np.fromfile(base(suite) + ".rec", np.uint32).reshape(-1, 32)
    ev = np.fromfile(base(suite) + ".events", np.uint32)
    assert len(cases) == len(rec) == len(ev) > 0
    return cases, rec, ev


def is_nan(words):
    return ((words & 0x7f800000) == 0x7f800000) & ((words & 0x007fffff) != 0)


def same_records(got, want, what):
    """Bit for bit, except that a NaN of the committed record only has to be a NaN."""
    got, want = np.asarray(got, np.uint32).reshape(-1, 32), np.asarray(want, np.uint32).reshape(-1, 32)
    assert got.shape == want.shape, what
    nan = is_nan(want)
    ok = np.where(nan, is_nan(got), got == want)
    bad = np.flatnonzero(~ok.all(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(got)} records differ, first case {bad[0]}, words {np.flatnonzero(~ok[bad[0]]).tolist()}: "
                           f"got {got[bad[0]].tolist()}, committed {want[bad[0]].tolist()}")


def run_shade(exe, suite, out, *extra, scene=None):
    return subprocess.run([exe, "shade", scene or base(suite) + ".yscn", base(suite) + ".txt", base(suite) + ".cases", str(out), *extra],
                          check=True, capture_output=True, text=True)


@pytest.fixture(scope="session")
def live_reference():
    """oracle/_ref/yart_ref where it is built and has the `shade` mode (its usage line names it), else None. A binary carried
    over from a tree that had no such mode is rebuilt first where the reference's sources are; without the sources the committed
    records, which are that reference's own, stand alone."""
    def has_shade():
        return os.path.exists(REF_BIN) and " shade " in subprocess.run([REF_BIN], capture_output=True, text=True).stderr
    if os.path.exists(REF_BIN) and not has_shade():
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], capture_output=True)
    return REF_BIN if has_shade() else None


# ------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("suite", shadesuite.SUITES)
def test_generator_reproduces_the_fixtures(suite, oracle_bin, tmp_path):
    from yart_amd import scenes
    s, p, cases = shadesuite.build(suite)
    assert s.tobytes() == open(base(suite) + ".yscn", "rb").read(), "scene"
    assert cases.tobytes() == open(base(suite) + ".cases", "rb").read(), "cases"
    scenes.write_params(tmp_path / "p.txt", p)
    assert open(tmp_path / "p.txt").read() == open(base(suite) + ".txt").read(), "params"
    assert np.isfinite(cases["f"]).all() and (cases["kind"] < 6).all() and not cases["pad"].any()
    assert all(t.width >= 2 and t.height >= 2 for t in s.textures)
    if suite == "lights":
        assert shadesuite.lights_scene(1).tobytes() == open(base(suite) + ".state2.yscn", "rb").read(), "second state"


def test_budgets():
    total = 0
    for suite in shadesuite.SUITES:
        n = os.path.getsize(base(suite) + ".cases") // shadesuite.CASE.itemsize
        assert n <= shadesuite.MAX_CASES
        total += n
    assert total <= shadesuite.MAX_CASES_ALL == 60000
    for name in os.listdir(SHADING):
        assert os.path.getsize(os.path.join(SHADING, name)) <= LARGEST_FIXTURE, name


@pytest.mark.parametrize("suite", shadesuite.SUITES)
def test_event_floors_and_nan_share(suite):
    """A suite meets the events it is aimed at, at least 64 cases each — a condition on the cases, not a measurement — and fewer
    than 1 % of the committed result words are NaN, so that the NaN rule of the comparison cannot hide a suite."""
    _, rec, ev = committed(suite)
    counts = json.load(open(base(suite) + ".events.json"))
    for k, name in enumerate(shadesuite.EVENTS):
        assert int(((ev >> k) & 1).sum()) == counts[name], name
    print(suite, counts)
    for name in shadesuite.TARGETS[suite]:
        assert counts[name] >= shadesuite.FLOOR >= 64, f"{suite}: {counts[name]} cases meet {name}, the floor is {shadesuite.FLOOR}"
    share = float(is_nan(rec).mean())
    print(f"{suite}: NaN share {100 * share:.3f} %")
    assert share < 0.01
    if suite == "lights":
        assert float(is_nan(np.fromfile(base(suite) + ".state2.rec", np.uint32)).mean()) < 0.01


def test_every_event_is_some_suites_target():
    assert sorted(e for t in shadesuite.TARGETS.values() for e in t) == sorted(shadesuite.EVENTS)


@pytest.mark.parametrize("suite", shadesuite.SUITES)
def test_oracle_and_reference_give_the_committed_records(suite, oracle_bin, live_reference, tmp_path):
    _, rec, ev = committed(suite)
    r = run_shade(oracle_bin, suite, tmp_path / "o.rec")
    same_records(np.fromfile(tmp_path / "o.rec", np.uint32), rec, f"{suite}: oracle")
    assert np.array_equal(np.fromfile(str(tmp_path / "o.rec") + ".events", np.uint32), ev), "event masks"
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.load(open(base(suite) + ".events.json")), "event counts"
    if live_reference:
        run_shade(live_reference, suite, tmp_path / "r.rec")
        same_records(np.fromfile(tmp_path / "r.rec", np.uint32), rec, f"{suite}: compiled reference")
    if suite == "lights":
        rec2 = np.fromfile(base(suite) + ".state2.rec", np.uint32)
        run_shade(oracle_bin, suite, tmp_path / "o2.rec", scene=base(suite) + ".state2.yscn")
        same_records(np.fromfile(tmp_path / "o2.rec", np.uint32), rec2, "lights, second state: oracle")
        if live_reference:
            run_shade(live_reference, suite, tmp_path / "r2.rec", scene=base(suite) + ".state2.yscn")
            same_records(np.fromfile(tmp_path / "r2.rec", np.uint32), rec2, "lights, second state: compiled reference")
        assert (rec2.reshape(-1, 32) != rec).any(), "the second state is another state"


@pytest.mark.parametrize("entries", [0, 1])
@pytest.mark.parametrize("suite", shadesuite.SUITES)
def test_hostsim_gives_the_committed_records(suite, entries, hostsim, tmp_path):
    """csrc/shade_record.hpp compiled for the host — the function k_probe_shading runs: entries 0 through bsdfF / bsdfPdf /
    bsdfSample, entries 1 through one matEvaluate and the *ImplE entries in the local frame, as wfShade calls them."""
    _, rec, _ = committed(suite)
    run_shade(hostsim, suite, tmp_path / "h.rec", str(entries))
    same_records(np.fromfile(tmp_path / "h.rec", np.uint32), rec, f"{suite}: hostsim, entries {entries}")
    if suite == "lights":
        run_shade(hostsim, suite, tmp_path / "h2.rec", str(entries), scene=base(suite) + ".state2.yscn")
        same_records(np.fromfile(tmp_path / "h2.rec", np.uint32), np.fromfile(base(suite) + ".state2.rec", np.uint32), "lights, second state: hostsim")


def test_hostsim_refuses_a_case_outside_the_scene(hostsim, tmp_path):
    cases, _, _ = committed("textures")
    bad = cases[:1].copy()
    bad["index"] = 1000
    bad.tofile(tmp_path / "bad.cases")
    r = subprocess.run([hostsim, "shade", base("textures") + ".yscn", base("textures") + ".txt", str(tmp_path / "bad.cases"), str(tmp_path / "o")],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "out of range" in r.stderr

    def refused(suite, cases, why):
        cases.tofile(tmp_path / "bad.cases")
        r = subprocess.run([hostsim, "shade", base(suite) + ".yscn", base(suite) + ".txt", str(tmp_path / "bad.cases"), str(tmp_path / "o")],
                           capture_output=True, text=True)
        assert r.returncode == 2 and why in r.stderr, (suite, why, r.stderr)
    for u in (1.0, 2.0, -0.5):                  # no area light in this scene: u >= 1 would index an empty power table
        refused("textures", shadesuite.case(shadesuite.PICK, 0, 0, (u,)), "[0, 1)")
    refused("luts", shadesuite.case(shadesuite.PICK, 0, 0, (0.5,)), "needs a scene with lights")
    refused("textures", np.frombuffer(cases[:2].tobytes()[:200], np.uint8), "multiple of")      # a truncated file
    s, _, _ = shadesuite.build("textures")
    m = s.materials[-1]
    assert [m.tex_base, m.tex_normal, m.tex_mr] == BUNDLE_TEXTURES


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


@pytest.mark.gpu
@pytest.mark.parametrize("quads", [True, False], ids=["footprint_records", "plain_texels"])
@pytest.mark.parametrize("suite", shadesuite.SUITES)
def test_device_probe_vs_committed_records(api, suite, quads, monkeypatch):
    """One DeviceScene per test, reading tests/golden only: every form of the probe gives the committed records."""
    cases, rec, _ = committed(suite)
    if not quads:
        monkeypatch.setenv("YART_TEX_QUADS_MAX_MB", "0")
    scene = api.DeviceScene(base(suite) + ".yscn", device=0)
    try:
        if suite == "textures":
            assert (len(scene.lighting_records()["tex_quads"]) > 0) == quads
        for form in FORMS:
            same_records(scene.probe_shading(cases, form), rec, f"{suite}: form {form}, {'footprint records' if quads else 'plain texels'}")
    finally:
        scene.close()


def kat_sections(cases, out):
    """The probe's records of hostsim's shade-kat-cases list, laid out as the KAT's ggx*, bsdf_f / bsdf_i and lights_f / lights_i
    sections (oracle/ref_driver.cpp doKat) — without the two per-light words the probe does not return (power)."""
    kind = cases["kind"]
    f = {}
    lut = out[kind == shadesuite.LUT]
    for k, name in enumerate(["ggxE", "ggxEavg", "ggxBaseE", "ggxBaseEavg", "ggxGlassE"]):
        f[name] = lut[:, k]
    b, m = out[kind == shadesuite.BSDF], out[kind == shadesuite.MAT]
    f["bsdf_f"] = np.concatenate([b[:, 1:16], m[:, 0:10]], axis=1).reshape(-1)
    f["bsdf_scatter"] = b[:, 0]
    li, pk = out[kind == shadesuite.LIGHT], out[kind == shadesuite.PICK]
    f["light_calls"] = li[:, 0:17]
    f["light_p"] = li[:, 17]
    f["pick_i"], f["pick_p"] = pk[:, 0], pk[:, 1]
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("name", KAT_GOLDENS)
def test_committed_kat_through_the_probe(api, name, hostsim, tmp_path):
    """The case list doKat evaluates (hostsim shade-kat-cases: the function `hostsim kat` itself iterates) through the probe, forms
    0 and 7, against the ggx*, bsdf_* and lights_* sections of the committed .kat.json — the compiled reference's own output —
    bit for bit (NaN for NaN)."""
    g = os.path.join(GOLDEN, name)
    subprocess.run([hostsim, "shade-kat-cases", g + ".yscn", g + ".txt", str(tmp_path / "k.cases")], check=True, capture_output=True)
    cases = np.fromfile(tmp_path / "k.cases", shadesuite.CASE)
    kat = json.load(open(g + ".kat.json"))
    U = lambda key: np.asarray(kat[key], np.uint32)
    n_b = int((cases["kind"] == shadesuite.BSDF).sum())
    n_l = int((cases["kind"] == shadesuite.LIGHT).sum()) // 4
    n_p = int((cases["kind"] == shadesuite.PICK).sum())
    assert n_b > 0 and len(kat["bsdf_f"]) == 25 * n_b and len(kat["lights_f"]) == 70 * n_l + n_p and len(kat["lights_i"]) == n_p

    def same(got, want, what):
        got, want = np.asarray(got, np.uint32).reshape(-1), np.asarray(want, np.uint32).reshape(-1)
        assert got.shape == want.shape, what
        ok = np.where(is_nan(want), is_nan(got), got == want)
        assert ok.all(), f"{name}, {what}: {int((~ok).sum())} words differ, first at {int(np.flatnonzero(~ok)[0])}"
    scene = api.DeviceScene(g + ".yscn", device=0)
    try:
        for form in (0, 7):
            f = kat_sections(cases, scene.probe_shading(cases, form))
            for key in ("ggxE", "ggxEavg", "ggxBaseE", "ggxBaseEavg", "ggxGlassE"):
                same(f[key], U(key), f"form {form}, {key}")
            same(f["bsdf_f"], U("bsdf_f"), f"form {form}, bsdf_f")
            n_mat = n_b // 48
            same(f["bsdf_scatter"], np.asarray(kat["bsdf_i"], np.int64).reshape(n_mat, 49)[:, :48].astype(np.uint32), f"form {form}, bsdf_i")
            lf = U("lights_f")
            per = lf[:70 * n_l].reshape(n_l, 70)
            same(f["light_calls"], per[:, 1:69], f"form {form}, lights_f (sample, pdf, Le)")
            same(f["light_p"].reshape(n_l, 4), np.repeat(per[:, 69:70], 4, axis=1), f"form {form}, lights_f (sampler p)")
            same(f["pick_p"], lf[70 * n_l:], f"form {form}, lights_f (pick p)")
            same(f["pick_i"], np.asarray(kat["lights_i"], np.int64).astype(np.uint32), f"form {form}, lights_i")
    finally:
        scene.close()


@pytest.mark.gpu
def test_tables_the_device_rebuilt(api):
    """The lights suite's scene moved to the second state of its maps and emissions through yart_hip_scene_update_lighting (the
    device rebuilds the environment tables and the power table itself): the probe gives the records the reference gives for a scene
    created in that state; moved back, the committed records of the first state again."""
    from yart_amd.yscn import Scene
    cases, rec, _ = committed("lights")
    rec2 = np.fromfile(base("lights") + ".state2.rec", np.uint32).reshape(-1, 32)
    s1, s2 = Scene.load(base("lights") + ".yscn"), Scene.load(base("lights") + ".state2.yscn")
    images = lambda s: {i: t.data for i, t in enumerate(s.textures) if t.is_float}
    scene = api.DeviceScene(base("lights") + ".yscn", device=0)
    try:
        same_records(scene.probe_shading(cases, 7), rec, "lights: as created")
        scene.update_lighting(materials=s2.materials, lights=s2.lights, images=images(s2))
        for form in (0, 7):
            same_records(scene.probe_shading(cases, form), rec2, f"lights: updated to the second state, form {form}")
        scene.update_lighting(materials=s1.materials, lights=s1.lights, images=images(s1))
        for form in (0, 7):
            same_records(scene.probe_shading(cases, form), rec, f"lights: restored to the first state, form {form}")
    finally:
        scene.close()


@pytest.mark.gpu
def test_probe_shading_refusals(api):
    import ctypes as C
    L = api.lib()
    cases, _, _ = committed("textures")
    one = np.ascontiguousarray(cases[:1])
    out = np.zeros(32, np.uint32)
    optr = out.ctypes.data_as(C.c_void_p)
    scene = api.DeviceScene(base("textures") + ".yscn", device=0)
    try:
        h = scene._h
        ptr = one.ctypes.data_as(C.c_void_p)
        assert L.yart_hip_probe_shading(None, 1, ptr, 0, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_shading(h, 1, None, 0, optr) == api.YART_E_INVALID
        assert L.yart_hip_probe_shading(h, 1, ptr, 0, None) == api.YART_E_INVALID
        assert L.yart_hip_probe_shading(h, 1, ptr, 8, optr) == api.YART_E_INVALID, "unknown form bit"
        assert L.yart_hip_probe_shading(h, (1 << 20) + 1, ptr, 0, optr) == api.YART_E_INVALID, "n"
        n_tex = len(scene.lighting_records()["textures"])
        for kind, index in ((6, 0), (shadesuite.TEX, n_tex), (shadesuite.MAT, 1000), (shadesuite.BSDF, 1000), (shadesuite.LIGHT, 4)):        # (the scene has four lights)
            bad = one.copy()
            bad["kind"], bad["index"] = kind, index
            assert L.yart_hip_probe_shading(h, 1, bad.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID, (kind, index)
        bad = one.copy()
        bad["f"][0, 0] = np.inf
        assert L.yart_hip_probe_shading(h, 1, bad.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID, "operand not finite"
        assert b"probe_shading" in L.yart_hip_last_error()
        # the light pick takes a sampler value: in this scene without area lights u >= 1 would index an empty power table
        for u in (1.0, 2.0, -0.5, float(np.nextafter(np.float32(1), np.float32(2)))):
            bad = shadesuite.case(shadesuite.PICK, 0, 0, (u,))
            assert L.yart_hip_probe_shading(h, 1, bad.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID, ("PICK", u)
            assert b"[0, 1)" in L.yart_hip_last_error()
        ok = shadesuite.case(shadesuite.PICK, 0, 0, (shadesuite.ONE_MINUS,))
        assert L.yart_hip_probe_shading(h, 1, ok.ctypes.data_as(C.c_void_p), 0, optr) == 0
        # the maps of the bundled material are sampled only through the bundle's clones: no footprint records of their own
        for tex in BUNDLE_TEXTURES:
            bad = shadesuite.case(shadesuite.TEX, tex, 0, (0.5, 0.5))
            assert L.yart_hip_probe_shading(h, 1, bad.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID, ("TEX", tex)
            assert b"footprint records" in L.yart_hip_last_error()
        dark = api.DeviceScene(base("luts") + ".yscn", device=0)       # a scene without lights
        try:
            pick = shadesuite.case(shadesuite.PICK, 0, 0, (0.5,))
            assert L.yart_hip_probe_shading(dark._h, 1, pick.ctypes.data_as(C.c_void_p), 0, optr) == api.YART_E_INVALID
            assert b"needs a scene with lights" in L.yart_hip_last_error()
        finally:
            dark.close()
        assert L.yart_hip_probe_shading(h, 0, ptr, 0, optr) == 0
        assert L.yart_hip_probe_shading(h, 1, ptr, 7, optr) == 0
    finally:
        scene.close()
