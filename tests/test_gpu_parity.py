"""GPU parity tests proper: everything goes through the C ABI (libyart_hip.so) on a real
MI355X and is compared with the reference's outputs.

Bar: bit-exact. Integer / index results (BVH arrays, hit triangle ids, ray counts) are exact, and so is every
floating-point framebuffer: the device evaluates the reference's operations in the reference's order, including
glibc's own sinf / cosf / logf / expf algorithms (csrc/ymath.hpp), so every frame is the reference's bit for bit
(conftest.bit_identical_or_drift; north_star's RMSE < 1e-3 is the fallback bar only under YART_ALLOW_LIBM_DRIFT=1,
for a box whose glibc selects other libm variants)."""
import os
import subprocess

import numpy as np
import pytest

from tests import katlib
from tests.conftest import GOLDEN, REF_BIN, bit_identical_or_drift
from tests.paramfile import load_params

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-3        # BASELINE.json north_star: per-pixel RMSE < 1e-3 (linear HDR)


def rmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2)))


@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


PIPELINE_FLAGS = {"wavefront": 0, "megakernel": 1, "wavefront+shade_sort": 2, "wavefront+general_trace": 4,
                  "wavefront+direct_sampler": 8, "wavefront+no_refill": 16, "wavefront+no_compaction": 32,
                  "wavefront+no_shade_sort": 64,
                  # rays the lean kernels hand over are traced again from the root instead of being resumed
                  "wavefront+no_resume": 128,
                  # a pool of path slots with path regeneration instead of one slot per path of the batch
                  "wavefront+path_pool": 512,
                  # scenes of 64 nodes and more take their candidate windows from the top-level hierarchy by default; the two
                  # forms without it: chunked candidate masks (kNodesChunked) / per-lane walk of the node list (kNodesWalk) by size (262144), the walk (65536)
                  "wavefront+node_masks": 262144, "wavefront+node_walk": 65536}


@pytest.mark.parametrize("pipeline", list(PIPELINE_FLAGS))
@pytest.mark.parametrize("case", ["cornell", "material", "cornell_waves", "uniform_sky", "two_skies"])
def test_framebuffer_vs_reference_golden(api, case, pipeline):
    """Every golden frame of the compiled reference x every pipeline variant: bit-identical (uniform_sky = the reference's
    other environment preset, UniformInfiniteLight; two_skies = an image and a uniform infinite light at once)."""
    base = os.path.join(GOLDEN, case)
    p = load_params(base + ".txt")
    scene = api.DeviceScene(base + ".yscn", device=0)
    img, st = scene.render(p, flags=PIPELINE_FLAGS[pipeline])
    ref = np.fromfile(base + ".f32", np.float32).reshape(img.shape)
    assert np.all(img[..., 3] == 1.0)
    bit_identical_or_drift(img, ref, f"{case}/{pipeline} rays={st['rays']}")
    scene.close()


@pytest.mark.parametrize("case", ["cornell", "material"])
def test_bvh_identical_to_reference(api, case):
    """The node array + index permutation the kernels traverse == the reference's (FNV-1a
    hashes recorded by oracle/ref_driver.cpp in the KAT file)."""
    base = os.path.join(GOLDEN, case)
    kat = katlib.load(base + ".kat.json")["bvh"]
    scene = api.DeviceScene(base + ".yscn", device=0)

    def fnv(b):
        h = 0xcbf29ce484222325
        for x in b:
            h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
        return h
    for m in range(len(kat) // 3):
        nodes, idx = scene.bvh(m)
        assert len(nodes) == kat[3 * m]
        assert fnv(nodes.tobytes()) == kat[3 * m + 1]
        assert fnv(idx.tobytes()) == kat[3 * m + 2]
    scene.close()


@pytest.mark.parametrize("case", ["cornell", "material"])
def test_per_sample_radiance_vs_reference(api, case):
    """Per-sample radiance of the probe pixels (device path) vs the reference's values."""
    base = os.path.join(GOLDEN, case)
    p = load_params(base + ".txt")
    kat = katlib.load(base + ".kat.json")
    ref = katlib.as_float(kat["radiance"]).reshape(-1, 3)
    xys = [(x, y, s) for (x, y) in p["probe_pixels"] for s in range(p["spp"])]
    scene = api.DeviceScene(base + ".yscn", device=0)
    got, rays = scene.probe_samples(p, xys)
    assert got.shape == ref.shape
    exact = np.all(got.view(np.uint32) == ref.view(np.uint32), axis=1).mean()
    close = np.all(np.isclose(got, ref, rtol=1e-4, atol=1e-5, equal_nan=True), axis=1).mean()
    print(f"{case}: samples bit-identical {exact:.3f}, within 1e-4 {close:.3f}, rays {rays} vs {kat['probe_rays'][0]}")
    # with glibc's libm algorithms on the device every sample is the reference's bit for bit on this pool; should a box select
    # other libm variants the frames drift to the 1e-8 regime and this is the first test to say so
    if os.environ.get("YART_ALLOW_LIBM_DRIFT"):
        assert exact > 0.99 and close > 0.999, "probe samples differ from the reference's"
    else:
        assert exact == 1.0, "probe samples differ from the reference's"
    assert rays == kat["probe_rays"][0]                     # an integer result: exact
    scene.close()


@pytest.mark.usefixtures("ref_bin")
def test_cornell_512_64spp_vs_reference_live(api, tmp_path):
    """BASELINE configs[1]: Cornell 512x512, 64 spp on 1 MI355X, RMSE vs the CPU reference."""
    from yart_amd import scenes
    s, p = scenes.cornell(512, 512, 64, 4)
    sp, pp, out = tmp_path / "c.yscn", tmp_path / "c.txt", tmp_path / "c.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([REF_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    img, st = scene.render(p)
    ref = np.fromfile(out, np.float32).reshape(img.shape)
    bit_identical_or_drift(img, ref, f"cornell 512x512x64 ({512 * 512 * 64 / st['ms_device'] * 1e-3:.1f} Msamples/s)")
    scene.close()


def test_tile_sharding_partitions_the_frame(api):
    """rank/world sharding inside the library: the two half-renders are disjoint, their sum is
    the full render bit for bit, and the pixel sets equal the host mirror in yart_amd.dist."""
    from yart_amd import dist as yd
    base = os.path.join(GOLDEN, "cornell")
    p = load_params(base + ".txt")
    scene = api.DeviceScene(base + ".yscn", device=0)
    full, _ = scene.render(p)
    parts = [scene.render(p, rank=r, world_size=2)[0] for r in range(2)]
    for r in range(2):
        assert np.array_equal(parts[r][..., 3] == 1.0, yd.pixel_mask(128, 128, 64, r, 2))
    assert np.array_equal((parts[0] + parts[1]).view(np.uint32), full.view(np.uint32))
    # finer sharding blocks (shard_tile) deal the same pixels differently; the sampler still only knows tile_size
    for shard, world in ((16, 3), (8, 5)):
        q = dict(p, shard_tile=shard)
        parts = [scene.render(q, rank=r, world_size=world)[0] for r in range(world)]
        for r in range(world):
            assert np.array_equal(parts[r][..., 3] == 1.0, yd.pixel_mask(128, 128, shard, r, world))
        assert np.array_equal(sum(parts).view(np.uint32), full.view(np.uint32))
    scene.close()


@pytest.mark.usefixtures("oracle_bin")
def test_material_scene_vs_oracle_live(api, tmp_path):
    """A non-golden size of the all-materials scene against the CPU oracle run on the spot."""
    from yart_amd import scenes
    oracle = os.path.join(os.path.dirname(REF_BIN), "..", "_build", "yart_oracle")
    s, p = scenes.material_test(160, 96, 32, 8)
    sp, pp, out = tmp_path / "m.yscn", tmp_path / "m.txt", tmp_path / "m.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([oracle, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    img, st = scene.render(p)
    ref = np.fromfile(out, np.float32).reshape(img.shape)
    bit_identical_or_drift(img, ref, "material 160x96x32")
    scene.close()


ORACLE_BIN = os.path.join(os.path.dirname(REF_BIN), "..", "_build", "yart_oracle")


@pytest.mark.usefixtures("oracle_bin")
@pytest.mark.parametrize("spp", [1, 2, 8, 12, 90, 300])
def test_sample_counts_vs_oracle_live(api, tmp_path, spp):
    """Sampler corner cases against the CPU oracle: 1 spp (no sample digits), odd log2spp (the
    'pow2Samples' last digit), non-power-of-two counts, and 90 spp (log2Int rounds DOWN to 6, so
    sample indices overflow the sampler's bit field: the per-render sampler tables must step aside)."""
    from yart_amd import scenes
    s, p = scenes.material_test(64, 48, spp, 6)
    sp, pp, out = tmp_path / "m.yscn", tmp_path / "m.txt", tmp_path / "m.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    img, _ = scene.render(p)
    ref = np.fromfile(out, np.float32).reshape(img.shape)
    # (1 spp: GMoN of a single bucket yields NaN pixels in the reference too: the comparison is on bits)
    bit_identical_or_drift(img, ref, f"material 64x48x{spp}")
    direct, _ = scene.render(p, flags=PIPELINE_FLAGS["wavefront+direct_sampler"])
    assert np.array_equal(img.view(np.uint32), direct.view(np.uint32)), "sampler tables changed a sample"
    scene.close()


def test_sponza_class_pipelines_agree(api):
    """The bench scene (alpha cut-outs, thin glass, nested transforms, env light) at a size the
    single-kernel integrator finishes in seconds: lean kernels + retry == general kernels ==
    megakernel, bit for bit; a second render reproduces the first (no order dependence left by
    the atomically filled queues)."""
    from yart_amd import scenes
    s, p = scenes.sponza_class(240, 136, 16, 8, tex=256, sky=256)
    scene = api.DeviceScene(s, device=0)
    a, st = scene.render(p)
    assert st["rays"] > 0 and np.isfinite(a).all()
    for name in ("megakernel", "wavefront+no_shade_sort", "wavefront+general_trace", "wavefront+no_refill", "wavefront+no_resume", "wavefront"):
        b, st2 = scene.render(p, flags=PIPELINE_FLAGS[name])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        assert st2["rays"] == st["rays"], name
    scene.close()


def test_resumed_walks_equal_restarted_walks(api, monkeypatch):
    """Rays the lean kernels hand to the general ones are taken up where the lean kernel stood (resume records: scene node,
    hit so far, leaf, traversal stack) — except shadow rays that are occluded already, rays with deep stacks and rays that find
    no record left, which are traced again from the root. Same frame whichever way a ray goes: all records, a few, none
    (YART_RESUME_CAP), and the flag that switches the records off; the counting build says how many rays went which way."""
    from yart_amd import scenes
    s, p = scenes.sponza_class(200, 112, 8, 8, tex=256, sky=256)
    scene = api.DeviceScene(s, device=0, instrumented=True)
    ref, st0 = scene.render(p, flags=PIPELINE_FLAGS["wavefront+no_resume"])
    c = scene.debug_counters()
    handed = int(c[29]) + int(c[30])
    assert handed > 1000 and int(c[8]) == 0 and int(c[9]) == 0
    seen = {}
    for cap in (None, "64", "0"):
        if cap is None:
            monkeypatch.delenv("YART_RESUME_CAP", raising=False)
        else:
            monkeypatch.setenv("YART_RESUME_CAP", cap)
        img, st = scene.render(p)
        c = scene.debug_counters()
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), f"YART_RESUME_CAP={cap}"
        assert st["rays"] == st0["rays"] and int(c[29]) + int(c[30]) == handed
        seen[cap] = (int(c[8]), int(c[9]))
    monkeypatch.delenv("YART_RESUME_CAP", raising=False)
    assert seen[None][0] > 0.9 * int(c[29]) and seen[None][1] > 0          # closest-hit rays: (nearly) all resumed
    assert 0 < sum(seen["64"]) < sum(seen[None])                             # a few records per launch, the rest restarted
    assert seen["0"] == (0, 0)
    scene.close()


@pytest.mark.usefixtures("oracle_bin")
@pytest.mark.parametrize("n_instances", [9, 70])
def test_alpha_candidates_inside_transformed_nodes_vs_oracle(api, tmp_path, n_instances):
    """Alpha cut-out "bushes" and thin-glass panes under rotated, non-uniformly scaled, nested nodes: the rays the lean kernels
    hand over stand inside transformed nodes, with and without an earlier hit, with some stack (9 instances: resume records;
    70: the many-node forms of the lean kernels, which restart). Every pipeline == the oracle, bit for bit."""
    from yart_amd import scenes
    s, p = scenes.alpha_instances(n_instances=n_instances)
    sp, pp, out = tmp_path / "a.yscn", tmp_path / "a.txt", tmp_path / "a.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0, instrumented=True)
    ref = None
    for name, flags in PIPELINE_FLAGS.items():
        img, st = scene.render(p, flags=flags)
        if ref is None:
            ref = np.fromfile(out, np.float32).reshape(img.shape)
        bit_identical_or_drift(img, ref, f"alpha_instances {len(s.nodes)} nodes / {name}")
        if name == "wavefront":
            c = scene.debug_counters()
            assert int(c[29]) > 100 and int(c[30]) > 100, "the scene must make the lean kernels hand rays over"
            if n_instances < 60:
                assert int(c[8]) > 0 and int(c[9]) > 0, "resume records must have been followed"
    scene.close()


@pytest.mark.usefixtures("oracle_bin")
def test_tables_larger_than_their_lds_slots_vs_oracle(api, tmp_path):
    """The shade kernel keeps the scene's small record tables in LDS where they fit (materials <= 64, texture descriptors <= 128,
    lights <= 8, ...); this scene has 96 materials, 160 textures and 26 area lights: every table stays in memory, and every
    pipeline must still reproduce the oracle bit for bit (scenes.many_records)."""
    from yart_amd import scenes
    s, p = scenes.many_records()
    assert len(s.materials) > 64 and len(s.textures) > 128 and len(s.lights) > 8
    sp, pp, out = tmp_path / "m.yscn", tmp_path / "m.txt", tmp_path / "m.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    ref = None
    for name, flags in PIPELINE_FLAGS.items():
        img, st = scene.render(p, flags=flags)
        if ref is None:
            ref = np.fromfile(out, np.float32).reshape(img.shape)
        bit_identical_or_drift(img, ref, f"many_records / {name}")
    scene.close()


def _vs_oracle(api, tmp_path, s, p, tag):
    from yart_amd import scenes
    sp, pp, out = tmp_path / "e.yscn", tmp_path / "e.txt", tmp_path / "e.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    img, st = scene.render(p)
    ref = np.fromfile(out, np.float32).reshape(img.shape)
    same, e = bit_identical_or_drift(img, ref, f"{tag} rays={st['rays']}")
    scene.close()
    return same, e


@pytest.mark.usefixtures("oracle_bin")
def test_edge_cases_vs_oracle_live(api, tmp_path):
    """Ragged and degenerate inputs against the CPU oracle: an image that is not a multiple of
    the 64-pixel tile (partial tiles in both directions, one of them a single pixel wide), a
    1x1 image, a scene without any light (only the background colour can arrive), a single
    bounce, and a deep bounce budget on the all-materials scene."""
    from yart_amd import scenes
    cases = []
    s, p = scenes.cornell(129, 65, 4, 4); cases.append(("cornell 129x65", s, p))
    s, p = scenes.cornell(1, 1, 4, 4); cases.append(("cornell 1x1", s, p))
    s, p = scenes.cornell(48, 48, 4, 4)
    s.lights = []
    for m in s.meshes:
        m.face_light = np.full(len(m.faces), -1, np.int32)
    p = dict(p, background=(0.25, 0.5, 0.75)); cases.append(("cornell without lights", s, p))
    s, p = scenes.material_test(64, 48, 4, 1); cases.append(("material depth 1", s, p))
    s, p = scenes.material_test(48, 32, 4, 24); cases.append(("material depth 24", s, p))
    for tag, s, p in cases:
        _vs_oracle(api, tmp_path, s, p, tag)


@pytest.mark.usefixtures("oracle_bin")
@pytest.mark.parametrize("n_instances", [20, 58, 70, 250, 600, 4200])
def test_instanced_scene_vs_oracle_live(api, tmp_path, n_instances):
    """Scene-graph walk: nested transformed group / instance nodes. 58 instances = exactly 64
    nodes (one window of the per-ray node candidate mask of trace_lean.hpp: the first size that leaves the
    kNodesMask form), 70 = 76 nodes (two windows), 250 = 256 nodes (four); 600 and 4200 instances: the sizes at which the forms without the top-level hierarchy
    switch to the per-lane walk, and at which the hierarchy's per-lane bitset needs word groups (more than 4096 nodes:
    the kNodesTlas form of trace_lean.hpp); every pipeline must reproduce the oracle."""
    from yart_amd import scenes
    s, p = scenes.instances(96, 96, 4, 4, n_instances=n_instances)
    sp, pp, out = tmp_path / "i.yscn", tmp_path / "i.txt", tmp_path / "i.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    ref = None
    for name, flags in PIPELINE_FLAGS.items():
        img, st = scene.render(p, flags=flags)
        if ref is None:
            ref = np.fromfile(out, np.float32).reshape(img.shape)
        bit_identical_or_drift(img, ref, f"instances {len(s.nodes)} nodes / {name}")
    scene.close()


@pytest.mark.usefixtures("oracle_bin")
def test_mclaren_class_waves_vs_oracle_live(api, tmp_path):
    """BASELINE configs[4] scene family (thin + refractive dielectric, clearcoat, DoF at f/2.8) at a
    size the CPU oracle finishes in a second, rendered as progressive waves (4 + 4 + 8 of 16 spp,
    blended as tile-renderer.hpp:220-232 does) and sharded over two ranks: the sum of the two
    half-frames must equal the oracle's frame."""
    from yart_amd import scenes
    s, p = scenes.mclaren_class(96, 54, 16, 8, detail=0.25, tex=64, sky=64)
    p = dict(p, first_wave=4, max_wave=8)
    sp, pp, out = tmp_path / "m.yscn", tmp_path / "m.txt", tmp_path / "m.f32"
    s.save(sp); scenes.write_params(pp, p)
    subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
    scene = api.DeviceScene(s, device=0)
    img, st = scene.render(p)
    ref = np.fromfile(out, np.float32).reshape(img.shape)
    assert st["waves"] == 3
    bit_identical_or_drift(img, ref, f"mclaren_class 96x54x16 in {st['waves']} waves")
    halves = [scene.render(p, rank=r, world_size=2)[0] for r in range(2)]
    assert np.array_equal((halves[0] + halves[1]).view(np.uint32), img.view(np.uint32))
    scene.close()


def test_full_size_properties(api):
    """BASELINE configs[2] at full size (1920x1080, 256 spp, 8 bounces; no CPU oracle finishes this in
    test time): size-independent properties of the renderer.
      * reproducibility: a second render is bit-identical (queues are filled with atomics, the result
        must not depend on their order);
      * partition: the frames of 8 tile-sharded ranks are disjoint and sum to the full frame, bit for bit;
      * linearity in exposure: +1 EV scales every sample by exactly 2 before GMoN, and GMoN (sums, sort
        by luma, Gini, trimmed mean) commutes with a power-of-two scale, so the frame doubles exactly;
      * every pixel finite with alpha 1;
      * hand-overs: the frame with the lean kernels' hand-overs resumed (the default: ~150 M resume records in this frame) equals the
        frame with every hand-over traced again from the root."""
    from yart_amd import scenes
    s, p = scenes.sponza_class(1920, 1080, 256, 8, tex=256, sky=512)
    scene = api.DeviceScene(s, device=0)
    full, st = scene.render(p)
    assert np.isfinite(full).all() and np.all(full[..., 3] == 1.0)
    assert st["samples"] == 1920 * 1080 * 256
    again, _ = scene.render(p)
    assert np.array_equal(full.view(np.uint32), again.view(np.uint32))
    restarted, st_r = scene.render(p, flags=PIPELINE_FLAGS["wavefront+no_resume"])
    assert np.array_equal(full.view(np.uint32), restarted.view(np.uint32)) and st_r["rays"] == st["rays"]
    acc = np.zeros_like(full)
    covered = np.zeros(full.shape[:2], np.int32)
    for r in range(8):
        part, _ = scene.render(p, rank=r, world_size=8)
        covered += (part[..., 3] == 1.0)
        acc += part
    assert np.all(covered == 1)
    assert np.array_equal(acc.view(np.uint32), full.view(np.uint32))
    brighter, _ = scene.render(dict(p, exposure=p["exposure"] + 1.0))
    assert np.array_equal((full[..., :3] * 2.0).view(np.uint32), brighter[..., :3].view(np.uint32))
    print(f"full size: {1920 * 1080 * 256 / st['ms_device'] * 1e-3:.1f} Msamples/s")
    scene.close()


def test_resumed_accumulation_equals_uninterrupted_render(api):
    """YartRenderParams.start_sample / stop_sample: rendering the first wave, handing the frame back and
    rendering the remaining waves must give the uninterrupted multi-wave render bit for bit (golden
    `cornell_waves`: 8 + 8 spp), including through the host-buffer entry point; a start that is not a
    wave boundary is rejected."""
    base = os.path.join(GOLDEN, "cornell_waves")
    p = load_params(base + ".txt")
    scene = api.DeviceScene(base + ".yscn", device=0)
    ref = np.fromfile(base + ".f32", np.float32).reshape(64, 64, 4)
    first, st1 = scene.render(dict(p, stop_sample=8))
    assert st1["waves"] == 1 and st1["samples"] == 64 * 64 * 8
    assert not np.array_equal(first.view(np.uint32), ref.view(np.uint32))
    rest, st2 = scene.render(dict(p, start_sample=8), accumulated=first)
    assert st2["waves"] == 1 and st2["samples"] == 64 * 64 * 8
    assert np.array_equal(rest.view(np.uint32), ref.view(np.uint32))
    with pytest.raises(api.YartError):
        scene.render(dict(p, start_sample=5), accumulated=first)
    scene.close()


def test_wave_callback_and_abort(api):
    """yart_hip_render_waves: the per-wave callback of Renderer::onRenderWaveComplete and abort between waves.
    cornell_waves = 16 spp as waves of 8 + 8 (the reference rendered its golden that way)."""
    base = os.path.join(GOLDEN, "cornell_waves")
    p = load_params(base + ".txt")
    ref = np.fromfile(base + ".f32", np.float32).reshape(p["size"][1], p["size"][0], 4)
    scene = api.DeviceScene(base + ".yscn", device=0)
    seen = []
    img, st, aborted = scene.render_waves(p, lambda frame, info: seen.append((dict(info), frame.copy())) and None)
    assert not aborted and st["waves"] == 2
    assert [s[0] for s in seen] == [dict(wave=0, wave_samples=8, samples_taken=8, total_samples=16),
                                    dict(wave=1, wave_samples=8, samples_taken=16, total_samples=16)]
    plain, _ = scene.render(p)
    assert np.array_equal(img.view(np.uint32), plain.view(np.uint32))
    bit_identical_or_drift(img, ref, "cornell_waves / render_waves")
    # the frame handed to the first callback is the render of the first wave alone
    first, _ = scene.render(dict(p, stop_sample=8))
    assert np.array_equal(seen[0][1].view(np.uint32), first.view(np.uint32))
    # abort after the first wave: that frame is returned
    img2, st2, aborted2 = scene.render_waves(p, lambda frame, info: True)
    assert aborted2 and st2["waves"] == 1 and np.array_equal(img2.view(np.uint32), first.view(np.uint32))
    # an exception in the callback stops the render and is re-raised
    class Boom(Exception):
        pass

    def bad(frame, info):
        raise Boom()
    with pytest.raises(Boom):
        scene.render_waves(p, bad)
    # no callback: same as render()
    img3, _, _ = scene.render_waves(p)
    assert np.array_equal(img3.view(np.uint32), plain.view(np.uint32))
    scene.close()


def test_python_tile_renderer_mirror(api):
    """api.HipTileRenderer: TileRenderer's knobs and calls (tile-renderer.hpp:25-115) on the Python side."""
    base = os.path.join(GOLDEN, "cornell_waves")
    p = load_params(base + ".txt")
    w, h = p["size"]
    ref = np.fromfile(base + ".f32", np.float32).reshape(h, w, 4)
    r = api.HipTileRenderer(w, h, {k: p[k] for k in ("focal", "fnumber", "eye", "target", "up", "exposure")})
    empty = r.render_sync()                                     # null scene: nothing happens (integrator.cpp:6)
    assert empty.samples_taken == 0 and not empty.buffer.any()
    r.scene = api.DeviceScene(base + ".yscn", device=0)
    r.samples, r.first_wave_samples, r.max_wave_samples, r.max_depth = p["spp"], p["first_wave"], p["max_wave"], p["depth"]
    waves = []
    r.on_render_wave_complete = lambda d, info: waves.append((d.samples_taken, info["wave_samples"]))
    done = []
    r.on_render_complete = done.append
    r.render(); r.wait()
    assert waves == [(8, 8), (16, 8)] and len(done) == 1 and done[0].samples_taken == 16
    bit_identical_or_drift(done[0].buffer, ref, "cornell_waves / HipTileRenderer")
    # abort from the wave callback's thread: the aborted callback fires with the first wave's frame
    aborted = []
    r.on_render_complete, r.on_render_aborted = None, aborted.append
    r.on_render_wave_complete = lambda d, info: r.abort()
    r.render(); r.wait()
    assert len(aborted) == 1 and aborted[0].samples_taken == 8
    # tonemapper: the exposed buffer is the AgX-mapped frame
    r.on_render_aborted = r.on_render_wave_complete = None
    r.tonemapper = "golden"
    mapped = r.render_sync()
    want, _ = api.tonemap(done[0].buffer, "golden")
    same = (mapped.buffer.view(np.uint32) == want.view(np.uint32)) | (np.isnan(mapped.buffer) & np.isnan(want))
    assert same.all()
    r.scene.close()


# oracle/kat_common.hpp:45-54 (the cases and the draw pattern of the KAT files' "sampler" section): (spp, tile, px, py, sample)
SAMPLER_CASES = [(16, 64, 3, 5, 7), (16, 64, 0, 0, 0), (16, 64, 255, 255, 15), (64, 64, 100, 37, 63), (256, 64, 1000, 700, 200),
                 (256, 64, 1919, 1079, 255), (1024, 64, 640, 360, 1023), (512, 64, 3839, 2159, 300), (8, 64, 17, 9, 5),
                 (32, 64, 77, 200, 31), (48, 64, 5, 6, 40), (16, 32, 40, 41, 3)]
SAMPLER_PATTERN = [2, 2, 2, 1, 1, 1, 2, 1, 2, 1, 1, 1, 2, 1, 1, 2]


@pytest.mark.parametrize("use_tables", [False, True])
def test_device_sampler_vs_reference_kat(api, use_tables):
    """The ZSobol / FastOwen sampler ON THE DEVICE (yart_hip_probe_sampler) against the compiled reference's draws (the "sampler"
    section of the committed KAT files: 12 (spp, pixel, sample) cases x 16 draws) and SURVEY §8(c)'s known answers, bit for bit —
    evaluated directly and through the per-render sampler tables the wavefront kernels read."""
    kat = katlib.as_float(katlib.load(os.path.join(GOLDEN, "cornell.kat.json"))["sampler"]).reshape(len(SAMPLER_CASES), -1)
    scene = api.DeviceScene(os.path.join(GOLDEN, "cornell.yscn"), device=0)
    for i, (spp, tile, px, py, smp) in enumerate(SAMPLER_CASES):
        got = scene.probe_sampler(spp, tile, [(px, py, smp)], SAMPLER_PATTERN, use_tables=use_tables)[0]
        assert np.array_equal(got.view(np.uint32), kat[i].view(np.uint32)), (SAMPLER_CASES[i], use_tables)
    # Sobol<FastOwen>(spp 16, res 64) pixel (3,5) sample 7; (spp 256) pixel (1000,700) sample 200
    a = scene.probe_sampler(16, 64, [(3, 5, 7)], [2, 1, 2], use_tables=use_tables)[0]
    assert np.array_equal(a, np.array([0.247990549, 0.85945183, 0.90101862, 0.263805777, 0.763566017], np.float32))
    b = scene.probe_sampler(256, 64, [(1000, 700, 200)], [2, 1], use_tables=use_tables)[0]
    assert np.array_equal(b, np.array([0.846162081, 0.899968386, 0.709087431], np.float32))
    # several cases in one call (the tables then hold one pixel column per case)
    same_spp = [c for c in SAMPLER_CASES if c[0] == 16 and c[1] == 64]
    many = scene.probe_sampler(16, 64, [c[2:] for c in same_spp], SAMPLER_PATTERN, use_tables=use_tables)
    for row, c in zip(many, same_spp):
        assert np.array_equal(row.view(np.uint32), kat[SAMPLER_CASES.index(c)].view(np.uint32))
    scene.close()


def test_texture_footprint_budget_fallback(api, monkeypatch):
    """The 2x2 footprint records of the textures are an optimisation with a memory budget (a third of the free device memory, or
    YART_TEX_QUADS_MAX_MB): a scene whose records do not fit keeps its plain texel arrays only and renders the same frame."""
    base = os.path.join(GOLDEN, "material")
    p = load_params(base + ".txt")
    ref = np.fromfile(base + ".f32", np.float32).reshape(p["size"][1], p["size"][0], 4)
    monkeypatch.setenv("YART_TEX_QUADS_MAX_MB", "0")
    scene = api.DeviceScene(base + ".yscn", device=0)
    img, _ = scene.render(p)
    bit_identical_or_drift(img, ref, "material / no footprint records")
    scene.close()
    from yart_amd import scenes
    s, q = scenes.sponza_class(160, 90, 4, 6, tex=128, sky=128)     # bundled base / normal / metal-rough maps, a float sky
    plain = api.DeviceScene(s, device=0)
    a, _ = plain.render(q)
    plain.close()
    monkeypatch.delenv("YART_TEX_QUADS_MAX_MB")
    full = api.DeviceScene(s, device=0)
    b, _ = full.render(q)
    full.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("pipeline", ["wavefront", "wavefront+path_pool", "wavefront+no_compaction"])
def test_batch_clamp_on_a_small_device_budget(api, pipeline, monkeypatch):
    """the batch fit bound counts what grows with the batch (path state, tail states, resume records) and takes the
    fixed allocations (sampler tables, spill / resume ranges) off the budget first; the path pool is clamped the same way. A fake
    budget of a few MB (YART_FAKE_FREE_MB, read per render) forces the clamp: the render must complete in several batches — not
    fail in hipMalloc — and give the golden frame."""
    base = os.path.join(GOLDEN, "cornell")
    p = load_params(base + ".txt")
    ref = np.fromfile(base + ".f32", np.float32).reshape(p["size"][1], p["size"][0], 4)
    scene = api.DeviceScene(base + ".yscn", device=0)
    monkeypatch.setenv("YART_FAKE_FREE_MB", "48")
    img, st = scene.render(p, flags=PIPELINE_FLAGS[pipeline])
    monkeypatch.delenv("YART_FAKE_FREE_MB")
    bit_identical_or_drift(img, ref, f"cornell/{pipeline} under a 48 MB budget")
    scene.close()


def test_render_stages_are_roctx_ranges(api, tmp_path):
    """SURVEY §5 "tracing": the stages of a render are roctx ranges (csrc/trace_ranges.hpp; the library is bound by name, YART_ROCTX_LIB
    names it). With a logging stand-in (tests/fake_roctx) a two-wave render must open `yart:render` once, inside it per wave `generate`
    and per bounce `bounce k` > `extend`, `shade`, `shadow` (+ `roulette`, `compact` from the second bounce on), then `gmon_blend`;
    every push has its pop, nesting never exceeds three levels — and the frame is still the golden one. Run in a child process: the
    library is bound once per process."""
    import sys
    from tests.conftest import ROOT
    so = str(tmp_path / "libfake_roctx.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(ROOT, "tests", "fake_roctx", "fake_roctx.c")], check=True)
    log = str(tmp_path / "roctx.log")
    base = os.path.join(GOLDEN, "cornell_waves")
    code = (f"import sys; sys.path.insert(0, {ROOT!r})\n"
            "import numpy as np\nfrom yart_amd import api\nfrom tests.paramfile import load_params\n"
            f"base = {base!r}\np = load_params(base + '.txt')\nds = api.DeviceScene(base + '.yscn', device=0)\nimg, st = ds.render(p)\n"
            "ref = np.fromfile(base + '.f32', np.float32).reshape(img.shape)\nassert np.array_equal(img.view(np.uint32), ref.view(np.uint32))\nds.close()\n")
    env = dict(os.environ, YART_ROCTX_LIB=so, FAKE_ROCTX_LOG=log)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = [ln.split(" ", 2) for ln in open(log).read().splitlines()]
    pushes = [ln[2] for ln in lines if ln[0] == "push"]
    assert sum(ln[0] == "push" for ln in lines) == sum(ln[0] == "pop" for ln in lines) and max(int(ln[1]) for ln in lines) <= 3
    assert pushes.count("yart:render") == 1 and pushes[0] == "yart:render" and lines[-1][0] == "pop" and lines[-1][1] == "0"
    depth = load_params(base + ".txt")["depth"]
    assert pushes.count("yart:sampler_tables") == 1 and pushes.count("yart:generate") == 2 and pushes.count("yart:gmon_blend") == 2   # two waves
    for k in range(depth):
        assert pushes.count(f"yart:bounce {k}") == 2
    assert pushes.count("yart:extend") == pushes.count("yart:shade") == pushes.count("yart:shadow") == 2 * depth
    assert pushes.count("yart:roulette") == 2 * max(0, depth - 2) and pushes.count("yart:compact") == 2 * max(0, depth - 2)
