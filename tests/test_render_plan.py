"""The launch plan of a render, pinned through YartStats (include/yart_hip.h): which pipeline ran, how many waves and
batches, and one launch per stage per bounce. Every expectation is worked out here from the header's definitions —
the wave schedule of YartRenderParams (samples / first_wave_samples / max_wave_samples), max_batch_paths, the
YART_FLAG_* values and what each YartStats counter sums — never taken from a run.

scenes.cornell at 20 x 12, 16 spp, depth 4: one rank owns all 240 pixels; first_wave = 1, max_wave = 4 gives the
waves 1, 1, 2, 4, 4, 4 (a lone first sample is followed by another single one, then the wave doubles up to max_wave)."""
import numpy as np
import pytest

from tests.test_gpu_parity import PIPELINE_FLAGS

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 20, 12, 16, 4
FIRST, MAX = 1, 4
PIXELS = W * H


@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


def schedule(samples, first, max_wave):
    """The waves of tile-renderer.hpp:121-124, 284-289: w0 = min(first, samples), then min(2 w, max) capped by what is
    left; a first wave of one sample is followed by another single one."""
    waves, taken, w = [], 0, min(first, samples)
    while w > 0:
        waves.append(w)
        taken += w
        nxt = min(2 * w, max_wave) if (len(waves) > 1 or w > 1) else 1
        w = min(nxt, samples - taken)
    return waves


WAVES = schedule(SPP, FIRST, MAX)
assert WAVES == [1, 1, 2, 4, 4, 4]


def batch_pixels(max_batch_paths):
    """Pixels per batch. max_batch_paths bounds the (pixel, sample) paths of a batch (0: 2^28), and the batch is one number
    of pixels for the whole render: the bound over the most samples a wave of this render can take — the larger of
    first_wave_samples and max_wave_samples, each capped by samples — at least one pixel, at most the rank's pixels; then
    the batches are made equal in size (the last one is not a sliver)."""
    bound = max_batch_paths if max_batch_paths else 1 << 28
    wave_cap = max(min(FIRST, SPP), min(MAX, SPP))
    chunk = min(PIXELS, max(bound // wave_cap, 1))
    if PIXELS > chunk:
        n_batches = -(-PIXELS // chunk)
        chunk = -(-PIXELS // n_batches)
    return chunk


def batches_per_wave(max_batch_paths):
    return -(-PIXELS // batch_pixels(max_batch_paths))


@pytest.fixture(scope="module")
def cornell(api):
    from yart_amd import scenes
    s, p = scenes.cornell(W, H, SPP, DEPTH)
    scene = api.DeviceScene(s, device=0)
    yield scene, dict(p, first_wave=FIRST, max_wave=MAX)
    scene.close()


@pytest.fixture(scope="module")
def whole(cornell):
    """The frame of one uninterrupted call (default pipeline): what every other way of rendering it must give."""
    scene, p = cornell
    img, st = scene.render(p)
    img.setflags(write=False)
    return img, st


def check_schedule(st, waves=WAVES):
    assert st["waves"] == len(waves)
    assert st["samples"] == PIXELS * sum(waves)


# 37 paths per batch = 9 pixels of the 4-sample waves -> 27 batches; 240 = 60 pixels -> 4 batches
@pytest.mark.parametrize("cap", [0, 240, 37])
@pytest.mark.parametrize("pipeline", ["wavefront", "wavefront+general_trace", "wavefront+no_refill", "wavefront+no_compaction"])
def test_batch_synchronous_launch_plan(cornell, whole, pipeline, cap):
    scene, p = cornell
    img, st = scene.render(dict(p, max_batch_paths=cap), flags=PIPELINE_FLAGS[pipeline])
    assert np.array_equal(img.view(np.uint32), whole[0].view(np.uint32))
    check_schedule(st)
    n = len(WAVES) * batches_per_wave(cap) * DEPTH           # every batch of every wave goes through every bounce
    print(pipeline, cap, {k: v for k, v in st.items() if k.startswith("launches")})
    assert st["launches_extend"] == st["launches_connect"] == st["launches_shade_kernel"] == n
    lean = 0 if pipeline == "wavefront+general_trace" else n
    assert st["launches_extend_lean"] == lean and st["launches_shadow_lean"] == lean
    assert st["launches_traverse"] == 2 * n
    assert st["paths_at_bounce"][0] == PIXELS * SPP
    assert st["rays"] == whole[1]["rays"]


@pytest.mark.parametrize("cap", [0, 240])
def test_megakernel_launch_plan(cornell, whole, cap):
    scene, p = cornell
    img, st = scene.render(dict(p, max_batch_paths=cap), flags=PIPELINE_FLAGS["megakernel"])
    assert np.array_equal(img.view(np.uint32), whole[0].view(np.uint32))
    check_schedule(st)
    assert st["launches_traverse"] == len(WAVES) * batches_per_wave(cap)
    for k in ("launches_extend", "launches_connect", "launches_shade_kernel", "launches_extend_lean", "launches_shadow_lean"):
        assert st[k] == 0, k
    assert st["paths_at_bounce"][0] == 0
    assert st["rays"] == whole[1]["rays"]


@pytest.mark.parametrize("cap, pool_paths", [(0, 0), (240, 64)])
def test_path_pool_launch_plan(cornell, whole, cap, pool_paths):
    scene, p = cornell
    img, st = scene.render(dict(p, max_batch_paths=cap, pool_paths=pool_paths), flags=PIPELINE_FLAGS["wavefront+path_pool"])
    assert np.array_equal(img.view(np.uint32), whole[0].view(np.uint32))
    check_schedule(st)
    # one extend, one shade and one shadow stage per round
    rounds = st["launches_extend"]
    assert rounds == st["launches_connect"] == st["launches_shade_kernel"]
    assert st["launches_traverse"] == st["launches_extend"] + st["launches_connect"]
    # A round takes every live path one bounce further and a slot carries one path, so a round does at most `slots`
    # path-bounces; the frame's path-bounces are the batch-synchronous pipeline's paths_at_bounce summed (the same paths:
    # the frames are bit-identical). The pool never has more slots than the batch has paths, rounded up to a wave of 64.
    # Every batch of every wave needs at least one round as well.
    largest_batch = batch_pixels(cap) * max(WAVES)
    slots = min(pool_paths if pool_paths else 1 << 25, (largest_batch + 63) // 64 * 64)
    path_bounces = sum(whole[1]["paths_at_bounce"])
    assert path_bounces >= PIXELS * SPP
    print("rounds", rounds, "path bounces", path_bounces, "slots", slots)
    assert rounds >= max(-(-path_bounces // slots), len(WAVES) * batches_per_wave(cap))
    assert st["paths_at_bounce"][0] == 0
    assert st["rays"] == whole[1]["rays"]


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel", "wavefront+path_pool"])
def test_two_calls_at_a_wave_boundary_give_the_single_call(cornell, whole, pipeline):
    scene, p = cornell
    flags = PIPELINE_FLAGS[pipeline]
    k = 3                                                     # the first three waves, then the rest
    cut = sum(WAVES[:k])
    first, st1 = scene.render(dict(p, stop_sample=cut), flags=flags)
    check_schedule(st1, WAVES[:k])
    both, st2 = scene.render(dict(p, start_sample=cut), flags=flags, accumulated=first)
    check_schedule(st2, WAVES[k:])
    assert np.array_equal(both.view(np.uint32), whole[0].view(np.uint32))
    assert st1["rays"] + st2["rays"] == whole[1]["rays"]


@pytest.mark.parametrize("key, value, message", [("start_sample", 3, "start_sample is not a wave boundary"),
                                                 ("stop_sample", 5, "stop_sample is not a wave boundary"),
                                                 ("stop_sample", 11, "stop_sample is not a wave boundary")])
def test_a_range_off_the_wave_boundaries_is_refused(api, cornell, key, value, message):
    scene, p = cornell
    boundaries = set(np.cumsum(WAVES).tolist())
    assert value not in boundaries
    with pytest.raises(api.YartError) as e:
        scene.render(dict(p, **{key: value}))
    assert str(e.value).endswith(message)
