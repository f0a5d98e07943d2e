"""The reference's four per-pixel estimators (core/estimator.hpp:29-198), selected by YartRenderParams.estimator.

CPU: csrc/estimator.hpp — the functions k_gmon_blend runs — compiled for the host (hostsim `estimator`) against the
reference's own classes on sample groups with fireflies, NaN / negative / infinite samples and empty buckets
(goldens tests/golden/estimator/, made by `yart_ref estimator`; live on random groups and on `sample_groups`, whose groups
have some buckets empty and others full). GPU: a render with each estimator equals those same functions applied to the
device's own per-sample radiances, bit for bit; and k_gmon_blend itself, launched on caller-supplied records
(api.probe_estimator), equals the reference's classes on the goldens, at every sample count from 1 to 160 (each bucket count,
each trip count of the unrolled load loop), at every place of a pixel in a workgroup, under an exposure scale, through the
pixels[] scatter and the wave blend, and sums the ray words."""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.paramfile import load_params

E = os.path.join(GOLDEN, "estimator")
SPPS = (1, 4, 5, 14, 15, 16, 25, 35, 64, 155, 256)
KINDS = {"gmon": 0, "mean": 1, "mon": 2, "gmonb": 3}


def same_bits_or_both_nan(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("spp", SPPS)
def test_estimator_functions_equal_reference_classes(hostsim, tmp_path, spp, kind):
    base = os.path.join(E, f"spp{spp}")
    out = os.path.join(tmp_path, "o.f32")
    subprocess.run([hostsim, "estimator", str(KINDS[kind]), str(spp), base + ".in.f32", out], check=True)
    got = np.fromfile(out, np.float32)
    want = np.fromfile(base + f".k{KINDS[kind]}.f32", np.float32)
    assert got.shape == want.shape and got.size == 24 * 3
    assert same_bits_or_both_nan(got, want), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))


REF_BIN = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "yart_ref")


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/yart_ref not built here")
@pytest.mark.parametrize("seed", range(12))
def test_estimator_functions_on_random_sample_groups(hostsim, tmp_path, seed):
    """Random sample groups (24 pixels x spp x rgb: 6 decades, zeros, fireflies, every third seed with NaN / negative / infinite
    samples, all-equal and all-zero groups) through the reference's own classes and csrc/estimator.hpp on the host, all four
    estimators (1200 such cases run once: all equal)."""
    rng = np.random.RandomState(seed)
    spp = int(rng.choice([1, 2, 3, 5, 6, 7, 9, 14, 15, 16, 17, 24, 25, 26, 33, 35, 64, 100, 155, 156, 256, 300]))
    x = np.exp(rng.uniform(-8, 6, (24, spp, 3))).astype(np.float32)
    m = rng.rand(24, spp, 3)
    x[m < 0.05] = 0
    x[(m > 0.05) & (m < 0.08)] *= np.float32(1e4)
    if seed % 3 == 0:
        x[(m > 0.10) & (m < 0.12)] = np.nan
        x[(m > 0.12) & (m < 0.14)] *= -1
        x[(m > 0.14) & (m < 0.15)] = np.inf
    if seed % 7 == 3:
        x[:] = x[:, :1]
    if seed % 11 == 5:
        x[:] = 0
    inp = os.path.join(tmp_path, "in.f32")
    x.tofile(inp)
    for kind in KINDS.values():
        outs = []
        for exe in (REF_BIN, hostsim):
            out = os.path.join(tmp_path, "o.f32")
            subprocess.run([exe, "estimator", str(kind), str(spp), inp, out], check=True)
            outs.append(np.fromfile(out, np.float32))
        assert outs[0].shape == outs[1].shape and same_bits_or_both_nan(outs[1], outs[0]), (seed, spp, kind)


def test_bad_estimator_is_rejected(built):
    from yart_amd import api
    L = api.lib()
    cam = api.CameraDesc(); cam.width = cam.height = 8
    rp = api.RenderParams(); rp.samples = rp.first_wave_samples = rp.max_wave_samples = 1
    rp.tile_size = 64; rp.max_depth = 1; rp.world_size = 1; rp.estimator = 4
    # validation happens before the scene is touched only when the scene pointer is non-null: use the render
    # entry with a null scene -> INVALID either way; the message names the first failed requirement
    assert L.yart_hip_render(None, api.C.byref(cam), api.C.byref(rp), None, None) == api.YART_E_INVALID


def _render_equals_functions(hostsim, tmp_path, kind, **over):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0
    base = os.path.join(GOLDEN, "material")
    p = dict(load_params(base + ".txt"), estimator=KINDS[kind], **over)
    w, h = p["size"]; spp = p["spp"]
    scene = api.DeviceScene(base + ".yscn", device=0)
    img, _ = scene.render(p)
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    rad, _ = scene.probe_samples(p, np.stack([xs, ys, ss], -1).reshape(-1, 3))
    scene.close()
    scale = np.exp2(np.float32(p.get("exposure", 0.0))).astype(np.float32)       # integrator.cpp:23
    smp = (rad.reshape(-1, 3).astype(np.float32) * scale).astype(np.float32)
    inp, out = os.path.join(tmp_path, "i.f32"), os.path.join(tmp_path, "o.f32")
    smp.tofile(inp)
    subprocess.run([hostsim, "estimator", str(KINDS[kind]), str(spp), inp, out], check=True)
    want = np.fromfile(out, np.float32).reshape(h, w, 3)
    assert same_bits_or_both_nan(img[..., :3], want)
    if kind != "gmon" and not over:
        ref = np.fromfile(base + ".f32", np.float32).reshape(h, w, 4)[..., :3]
        assert not np.array_equal(img[..., :3], ref)                              # a different estimator, a different frame


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_render_with_estimator_equals_functions_on_device_samples(hostsim, tmp_path, kind):
    _render_equals_functions(hostsim, tmp_path, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_render_with_estimator_equals_functions_on_device_samples_7_buckets(hostsim, tmp_path, kind):
    """The same at 35 spp (7 buckets; the 16 spp of the scene's file give 3), on a quarter of the frame."""
    _render_equals_functions(hostsim, tmp_path, kind, spp=35, size=(48, 32))


# ---------------------------------------------------------------------------------------------------------------------
# k_gmon_blend itself (api.probe_estimator) against the reference's classes
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = 24
SEED = 7
# every bucket count (3 from 15 spp on, then two more every 10 up to the cap of 15 at 75) and, for each of them, every trip count
# of the kernel's unrolled loop (0, 1, 2+ rounds of four) and of its remainder (0-3 samples); the large counts for many rounds
SWEEP = tuple(range(1, 161)) + (255, 256, 257, 300, 1000)
# the host comparison: a stride through the sweep, each threshold of the bucket formula with the count before it, the large counts
STRIDED = tuple(sorted(set(range(1, 161, 7)) | {t - d for t in range(15, 146, 10) for d in (0, 1)} | {255, 256, 257, 300, 1000}))


def buckets(spp):
    """m of core/estimator.hpp:56 / :97 / :151 with mMax = 15 (the division truncates toward zero)."""
    return min(15, max(1, 1 + 2 * int((spp - 5) / 10)))


def sample_groups(spp, seed):
    """24 groups of spp RGB samples [24, spp, 3] float32. Every family sits at fixed group indices, so every call has all of them:
    0-3 benign values over six decades; 4, 5 fireflies (x 1e4); 6-8 NaN, negative and infinite values sprinkled in (8 also with
    fireflies and -Inf); 9 all samples equal; 10 all zero; 11 denormals (around 1e-42); 12, 13 values near 3e38 whose bucket sums
    overflow (13 mixed with benign ones); 14 wholly rejected (a NaN in every sample); 21 negative values only; 22 infinite values
    only; 23 half zeros, some of them -0. Where the sample count gives more than one bucket (bucket b = samples k with k mod m == b):
    15 exactly one bucket all NaN; 16 every bucket but one all negative; 17 every bucket but one all NaN; 18 one bucket with a single
    accepted sample among NaNs; 19 exactly one bucket all negative; 20 one bucket all NaN among fireflies. With one bucket, 15-20 are
    sprinkled like 6-8."""
    rng = np.random.RandomState([seed, spp])
    m = buckets(spp)
    x = np.exp(rng.uniform(-8, 6, (GROUPS, spp, 3))).astype(np.float32)
    u = rng.rand(GROUPS, spp, 3)
    k = np.arange(spp)

    def sprinkle(g, nan=0.0, neg=0.0, inf=0.0, fire=0.0, ninf=0.0, zero=0.0):
        at = 0.0
        for share, fn in ((nan, lambda v: np.nan), (neg, lambda v: -v), (inf, lambda v: np.inf), (fire, lambda v: np.maximum(v, 1) * np.float32(1e4)),
                          (ninf, lambda v: -np.inf), (zero, lambda v: 0.0)):
            sel = (u[g] >= at) & (u[g] < at + share)
            x[g][sel] = fn(x[g][sel])
            at += share

    sprinkle(4, fire=0.03); sprinkle(5, fire=0.10)
    for g in (4, 5):                                                                     # at least one, whatever the sample count
        x[g, rng.randint(spp), rng.randint(3)] = np.float32(1e4) * np.exp(rng.uniform(0, 6))
    sprinkle(6, nan=0.02, neg=0.02, inf=0.01)
    sprinkle(7, nan=0.10, neg=0.10, inf=0.05)
    sprinkle(8, nan=0.05, neg=0.05, inf=0.03, fire=0.05, ninf=0.03)
    x[9] = x[9, :1]
    x[10] = 0
    x[11] = rng.randint(1, 2000, (spp, 3)).astype(np.uint32).view(np.float32)              # 1.4e-45 .. 2.8e-42
    x[12] = rng.uniform(1e38, 3.4e38, (spp, 3)).astype(np.float32)
    x[13] = np.where(u[13] < 0.5, rng.uniform(1e38, 3.4e38, (spp, 3)).astype(np.float32), x[13])
    x[14, k, rng.randint(0, 3, spp)] = np.nan
    if m > 1:
        b = rng.randint(0, m, 6)
        x[15, k % m == b[0]] = np.nan
        x[16, k % m != b[1]] *= -1
        x[17, k % m != b[2]] = np.nan
        mine = k[k % m == b[3]]
        x[18, mine[mine != rng.choice(mine)]] = np.nan
        x[19, k % m == b[4]] *= -1
        sprinkle(20, fire=0.08); x[20, k % m == b[5]] = np.nan
    else:
        for i, g in enumerate(range(15, 21)):
            sprinkle(g, nan=0.03 * (i + 1), neg=0.03 * (6 - i), inf=0.01 * i)
    sprinkle(21, neg=0.30)
    sprinkle(22, inf=0.03)
    sprinkle(23, zero=0.5); x[23][(u[23] >= 0.5) & (u[23] < 0.55)] = -0.0
    return x


def empty_buckets(x, gmon_rule):
    """Per group of x [groups, spp, 3]: the accepted samples of every bucket [groups, m] under the acceptance rule of GMoN (a NaN or a
    negative channel rejects the sample, core/estimator.hpp:155) or of the other three (a NaN does, :35 / :60 / :101)."""
    spp = x.shape[1]; m = buckets(spp)
    bad = np.isnan(x).any(-1)
    if gmon_rule:
        bad |= (x < 0).any(-1)
    return np.stack([(~bad[:, b::m]).sum(1) for b in range(m)], 1)


def blend(h, v, wc, ww):
    """current * wCurrent + wave * wWave (tile-renderer.hpp:230) as k_gmon_blend states it: two rounded products, one rounded sum."""
    f = np.float32
    with np.errstate(all="ignore"):
        return (np.asarray(h, f) * f(wc)).astype(f) + (np.asarray(v, f) * f(ww)).astype(f)


def on_cleared_frame(v):
    """What the probe's defaults (a zero frame, weights (0, 1)) make of the estimate v: v itself, but for -0, which 0 * 0 + -0 * 1 turns
    into +0."""
    return blend(np.float32(0), v, 0.0, 1.0)


def mismatches(got, want):
    """Indices along the first axis where got and want differ in bits (a NaN may be another NaN)."""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~same.reshape(len(same), -1).all(1))


def run_estimator(exe, kind, x, tmp, tag):
    """`exe estimator` (yart_ref or hostsim) on the groups x [groups, spp, 3] -> [groups, 3]."""
    x = np.ascontiguousarray(x, np.float32)
    inp, out = os.path.join(tmp, f"{tag}.in.f32"), os.path.join(tmp, f"{tag}.out.f32")
    x.tofile(inp)
    subprocess.run([exe, "estimator", str(kind), str(x.shape[1]), inp, out], check=True)
    return np.fromfile(out, np.float32).reshape(x.shape[0], 3)


@pytest.mark.parametrize("gmon_rule", (True, False), ids=("gmon-rule", "nan-rule"))
def test_sample_groups_hold_their_families(gmon_rule):
    """From the inputs alone: at every sample count of the sweep with more than one bucket, under either acceptance rule, there are
    groups with exactly one empty bucket, with every bucket but one empty and with none empty; a wholly rejected group; a bucket
    with a single accepted sample; and the fixed families are what their index says."""
    for spp in SWEEP:
        x = sample_groups(spp, SEED)
        assert x.shape == (GROUPS, spp, 3) and x.dtype == np.float32
        assert same_bits_or_both_nan(x, sample_groups(spp, SEED))
        cnt = empty_buckets(x, gmon_rule)
        m = cnt.shape[1]
        assert m == buckets(spp)
        empties = (cnt == 0).sum(1)
        assert empties[14] == m, spp                                             # the wholly rejected group
        assert empties[0] == 0 and np.isfinite(x[:6]).all() and (x[:6] > 0).all(), spp
        assert (x[4] >= 1e4).any() and (x[5] >= 1e4).any() and (x[:4] < 404).all(), spp      # benign values end at e^6 = 403
        assert np.all(x[9] == x[9, 0]) and not x[10].any(), spp
        assert (x[11] > 0).all() and (x[11] < 1e-41).all(), spp
        assert (x[12] >= 1e38).all() and np.isfinite(x[12]).all(), spp
        if m > 1:
            with np.errstate(over="ignore"):
                assert all(np.isinf(x[12, b::m].sum(0, dtype=np.float32)).all() for b in range(m)), spp
            assert (empties == 1).sum() >= 1 and (empties == m - 1).sum() >= 1 and (empties == 0).sum() >= 1, (spp, empties)
            assert empties[15] == 1 and empties[17] == m - 1 and empties[20] == 1, (spp, empties)
            assert empties[16] == (m - 1 if gmon_rule else 0) and empties[19] == (1 if gmon_rule else 0), (spp, empties)
            assert empties[18] == 0 and (cnt[18] == 1).sum() == 1, (spp, cnt[18])


def test_bucket_formula_thresholds():
    assert [buckets(n) for n in (1, 4, 5, 14, 15, 24, 25, 64, 65, 74, 75, 145, 1000)] == [1, 1, 1, 1, 3, 3, 5, 11, 13, 13, 15, 15, 15]
    assert {t for t in range(2, 200) if buckets(t) != buckets(t - 1)} == set(range(15, 76, 10)) <= set(STRIDED)
    assert set(STRIDED) <= set(SWEEP)


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/yart_ref not built here")
def test_estimator_functions_equal_reference_classes_on_sample_groups(hostsim, tmp_path):
    """The groups of the device sweep — some buckets empty and others full, overflowing sums, denormals — through the reference's own
    classes and csrc/estimator.hpp on the host, all four estimators, at a stride through the sweep that holds every threshold of the
    bucket formula."""
    def one(job):
        spp, kind = job
        x = sample_groups(spp, SEED)
        want = run_estimator(REF_BIN, kind, x, tmp_path, f"ref{spp}k{kind}")
        got = run_estimator(hostsim, kind, x, tmp_path, f"host{spp}k{kind}")
        return [(kind, spp, int(g)) for g in mismatches(got, want)]
    with ThreadPoolExecutor(4) as pool:
        bad = sum(pool.map(one, [(spp, kind) for spp in STRIDED for kind in KINDS.values()]), [])
    assert not bad, f"{len(bad)} (kind, spp, group) differ between the reference and csrc/estimator.hpp: {bad[:40]}"


def test_probe_estimator_abi_and_argument_errors(built):
    """The symbol exists and is in api.EXPORTS, the ABI version is still 3, every argument error is YART_E_INVALID with a message that
    names it — decided before any device is touched — and without a device a well-formed call is YART_E_NO_DEVICE."""
    from yart_amd import api
    L = api.lib()
    assert hasattr(ctypes.CDLL(api.LIB_PATH), "yart_hip_probe_estimator")
    assert "yart_hip_probe_estimator" in api.EXPORTS
    assert L.yart_hip_abi_version() == 3
    rec = np.ones((4, 4, 4), np.float32)
    hdr = np.zeros((2, 2, 4), np.float32)
    rays = np.zeros(4, np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = dict(L_rgba=ptr(rec), n_pixels=4, spp=4, kind=0, exposure_scale=1.0, pixels=None, width=2, height=2, w_current=0.0, w_wave=1.0,
                hdr_inout=ptr(hdr), pix_rays=ptr(rays))

    def call(**over):
        return L.yart_hip_probe_estimator(*dict(good, **over).values())

    outside = [np.array([0, 1, 1 << 16, v], np.uint32) for v in (2, 2 << 16, 0xffff, 0xffff0000)]
    cases = [(dict(L_rgba=None), b"null"), (dict(hdr_inout=None), b"null"),
             (dict(n_pixels=0), b"n_pixels"), (dict(spp=0), b"spp"), (dict(width=0), b"width"), (dict(height=0), b"height"),
             (dict(kind=-1), b"kind"), (dict(kind=4), b"kind"),
             (dict(n_pixels=8193, spp=8192, width=8193, height=1), b"2^26"), (dict(n_pixels=1 << 26, spp=2, width=1 << 13, height=1 << 13), b"2^26"),
             (dict(width=65537, height=1), b"65536"), (dict(width=1, height=65537), b"65536"),
             (dict(n_pixels=5), b"width * height"), (dict(width=1), b"width * height"),
             (dict(exposure_scale=float("nan")), b"exposure_scale"), (dict(exposure_scale=float("inf")), b"exposure_scale"),
             (dict(w_current=float("-inf")), b"weight"), (dict(w_wave=float("nan")), b"weight")]
    cases += [(dict(pixels=ptr(px)), b"outside the frame") for px in outside]
    for over, word in cases:
        assert call(**over) == api.YART_E_INVALID, over
        assert word in L.yart_hip_last_error(), (over, L.yart_hip_last_error())
    assert not hdr.any() and not rays.any()
    if L.yart_hip_device_count() == 0:
        assert call() == api.YART_E_NO_DEVICE
        back = np.array([1 | 1 << 16, 1 << 16, 1, 0], np.uint32)
        assert call(pix_rays=None, pixels=ptr(back)) == api.YART_E_NO_DEVICE
        with pytest.raises(api.YartError) as e:
            api.probe_estimator(np.ones((3, 5, 3), np.float32), 2)
        assert e.value.code == api.YART_E_NO_DEVICE


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernel"
    return api


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """reference(kind, spp, scale=None) -> [24, 3]: `yart_ref estimator` on sample_groups(spp, SEED) (times scale, rounded to float32:
    the kernel's one product per channel); computed once per argument set for the whole module and never written to."""
    if not os.path.exists(REF_BIN):
        pytest.fail("oracle/_ref/yart_ref is missing: the estimator probe tests compare against it")
    tmp = str(tmp_path_factory.mktemp("estimator_ref"))
    cache = {}

    def get(kind, spp, scale=None):
        key = (kind, spp, None if scale is None else float(scale))
        if key not in cache:
            x = sample_groups(spp, SEED)
            if scale is not None:
                with np.errstate(all="ignore"):
                    x = (x * np.float32(scale)).astype(np.float32)
            v = run_estimator(REF_BIN, kind, x, tmp, "k%d.spp%d.s%s" % key)
            v.setflags(write=False)
            cache[key] = v
        return cache[key]

    def many(jobs):
        with ThreadPoolExecutor(8) as pool:
            return list(pool.map(lambda j: get(*j), jobs))
    get.many = many
    return get


def probe_groups(api, x, kind, **kw):
    """The probe on the groups x [n, spp, 3] as an n x 1 frame -> (rgb [n, 3], alpha [n], pix_rays [n])."""
    frame, rays = api.probe_estimator(x, kind, **kw)
    assert frame.shape == (1, len(x), 4) and frame.dtype == np.float32 and rays.shape == (len(x),)
    return frame[0, :, :3], frame[0, :, 3], rays


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_probe_estimator_equals_goldens(gpu_api, kind):
    """k_gmon_blend on the committed sample groups == the reference's classes' committed values, 11 sample counts x 24 pixels."""
    bad = []
    for spp in SPPS:
        base = os.path.join(E, f"spp{spp}")
        x = np.fromfile(base + ".in.f32", np.float32).reshape(GROUPS, spp, 3)
        want = np.fromfile(base + f".k{KINDS[kind]}.f32", np.float32).reshape(GROUPS, 3)
        rgb, alpha, _ = probe_groups(gpu_api, x, KINDS[kind])
        bad += [(kind, spp, int(g)) for g in mismatches(rgb, want)]
        assert np.array_equal(alpha.view(np.uint32), np.ones(GROUPS, np.float32).view(np.uint32)), (kind, spp)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_probe_estimator_sample_count_sweep(gpu_api, reference, kind):
    """Every sample count from 1 to 160, and 255, 256, 257, 300, 1000: each bucket count with each trip count of the kernel's unrolled
    loop and its remainder, on sample_groups, against the compiled reference run live. 165 x 24 (spp, group) cases per estimator."""
    want = reference.many([(KINDS[kind], spp) for spp in SWEEP])
    bad, cases = [], 0
    for spp, w in zip(SWEEP, want):
        rgb, alpha, _ = probe_groups(gpu_api, sample_groups(spp, SEED), KINDS[kind])
        bad += [(kind, spp, int(g)) for g in mismatches(rgb, on_cleared_frame(w))]
        assert np.all(alpha == 1), (kind, spp)
        cases += len(w)
    print(f"estimator sweep {kind}: {cases} (kind, spp, group) cases, {len(bad)} mismatches")
    assert cases == len(SWEEP) * GROUPS
    assert not bad, f"{len(bad)} of {cases} (kind, spp, group) differ from the reference: {bad[:60]}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("gmon", "mon"))
@pytest.mark.parametrize("spp", (35, 155))
def test_probe_estimator_workgroup_partition(gpu_api, reference, spp, kind):
    """1, 15, 16, 17 and 1000 pixels (16 share a workgroup): pixel i holds group i mod 24, and its value is the reference's for that
    group wherever it sits in its workgroup and whether or not the last workgroup is full."""
    want = on_cleared_frame(reference(KINDS[kind], spp))
    groups = sample_groups(spp, SEED)
    for n in (1, 15, 16, 17, 1000):
        which = np.arange(n) % GROUPS
        rgb, alpha, _ = probe_groups(gpu_api, groups[which], KINDS[kind])
        bad = mismatches(rgb, want[which])
        assert not len(bad), (kind, spp, n, [(int(i), int(i % GROUPS)) for i in bad[:40]])
        assert np.all(alpha == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_probe_estimator_exposure_scale(gpu_api, reference, kind):
    """The kernel multiplies every channel by the exposure scale once, rounded to float32, before anything else: the reference's
    classes fed those products."""
    bad = []
    for scale in (np.float32(2 ** -1.5), 3.7):
        for spp in (16, 35, 256):
            want = on_cleared_frame(reference(KINDS[kind], spp, scale))
            rgb, alpha, _ = probe_groups(gpu_api, sample_groups(spp, SEED), KINDS[kind], exposure_scale=scale)
            bad += [(kind, float(scale), spp, int(g)) for g in mismatches(rgb, want)]
            assert np.all(alpha == 1)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_probe_estimator_scatter_and_wave_blend(gpu_api, reference, kind):
    """19 pixels of a 7 x 5 frame in shuffled order: each goes to its pixels[] place as current * wCurrent + wave * wWave — two
    rounded products and a rounded sum per channel, so a fused multiply-add fails this — with alpha blended towards 1; the 16 other
    pixels keep their bits. The current frame holds zeros, a NaN and an Inf among seeded values."""
    w, h, n, spp = 7, 5, 19, 35
    rng = np.random.RandomState(11)
    where = rng.permutation(w * h)
    listed, others = where[:n], where[n:]
    xy = np.stack([listed % w, listed // w], 1)
    current = np.exp(rng.uniform(-6, 6, (h, w, 4))).astype(np.float32)
    flat = current.reshape(-1, 4)
    flat[listed[0]] = 0; flat[listed[1], 1] = np.nan; flat[listed[2], 2] = np.inf; flat[listed[3], 0] = -0.0
    flat[others[0]] = 0; flat[others[1], 0] = np.nan; flat[others[2], 3] = np.inf; flat[others[3], 1] = -0.0
    flat.view(np.uint32)[others[4], 2] = 0x7fc00123                                   # a NaN with a payload: kept as it is
    before = current.copy()
    v = reference(KINDS[kind], spp)[:n]
    x = sample_groups(spp, SEED)[:n]
    for wc, ww in [(0.0, 1.0), (0.25, 0.75)] + [(k / (k + 4), 4 / (k + 4)) for k in (4, 12)]:
        frame, _ = gpu_api.probe_estimator(x, KINDS[kind], pixels=xy, size=(w, h), current=current, weights=(wc, ww))
        assert np.array_equal(current.view(np.uint32), before.view(np.uint32))           # the caller's frame is not written
        got = frame.reshape(-1, 4)
        want = np.concatenate([blend(before.reshape(-1, 4)[listed, :3], v, wc, ww),
                               blend(before.reshape(-1, 4)[listed, 3:], np.ones((n, 1), np.float32), wc, ww)], 1)
        bad = mismatches(got[listed], want)
        assert not len(bad), (kind, wc, ww, [(int(i), got[listed][i], want[i]) for i in bad[:8]])
        assert np.array_equal(got[others].view(np.uint32), before.reshape(-1, 4)[others].view(np.uint32)), (kind, wc, ww)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("gmon", "mean", "gmonb"))
def test_probe_estimator_ray_counts(gpu_api, reference, kind):
    """The fourth word of a record is a ray count, not a float: whatever its bits (a float NaN, an Inf, 0), a pixel's count is the sum
    of its words mod 2^32, over every bucket's lane, and the radiance does not depend on them. A NULL pix_rays is accepted."""
    rng = np.random.RandomState(5)
    for spp in (1, 16, 35, 157, 300):
        x = sample_groups(spp, SEED)
        rays = rng.randint(0, 1 << 32, (GROUPS, spp), dtype=np.uint64).astype(np.uint32)
        sel = rng.rand(GROUPS, spp)
        rays[sel < 0.1] = 0x7fc00001; rays[(sel >= 0.1) & (sel < 0.2)] = 0x7f800000; rays[(sel >= 0.2) & (sel < 0.4)] = 0
        rays[(sel >= 0.4) & (sel < 0.45)] = 0xffffffff
        rays[3] = 0; rays[4] = rng.randint(0, 200, spp)                                    # what a render holds
        rgb, alpha, got = probe_groups(gpu_api, x, KINDS[kind], rays=rays)
        want = (rays.astype(np.uint64).sum(1) & 0xffffffff).astype(np.uint32)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (kind, spp, np.flatnonzero(got != want))
        plain, _, zero = probe_groups(gpu_api, x, KINDS[kind])
        assert not zero.any()
        assert not len(mismatches(rgb, plain)) and not len(mismatches(rgb, on_cleared_frame(reference(KINDS[kind], spp)))), (kind, spp)
        # the C entry with pix_rays == NULL
        rec = np.zeros((GROUPS, spp, 4), np.float32)
        rec[..., :3] = x; rec.view(np.uint32)[..., 3] = rays
        hdr = np.zeros((1, GROUPS, 4), np.float32)
        L = gpu_api.lib()
        assert L.yart_hip_probe_estimator(rec.ctypes.data_as(ctypes.c_void_p), GROUPS, spp, KINDS[kind], 1.0, None, GROUPS, 1, 0.0, 1.0,
                                          hdr.ctypes.data_as(ctypes.c_void_p), None) == gpu_api.YART_OK
        assert not len(mismatches(hdr[0, :, :3], rgb)) and np.all(hdr[0, :, 3] == 1)
