"""Device time of the per-pixel motion path at 1920 x 1080 (profiles/pixel_motion.txt).

The scene is profiles/mesh_update.txt's: scenes.heightfield(n=256), whose 131 k-triangle height field deforms (its vertices scaled a
little, two sets in turn), seen from above so that most pixels show it. Per frame, as an animation runs it: keep_previous,
update_meshes, a 1 spp render with the feature buffers into device tensors, pixel_motion_into, accumulate_into(pixel_motion=) — all
on torch's current stream. Timed with device events
around each call (every call returns after its work has completed on the stream) and, next to them, the wall time of the call; two
warm-up frames, then the median of 11. update_meshes' own device time (its statistics) is printed for comparison, and the accumulate
call without a motion.

    python tools/pixel_motion_trace.py [--out profiles/pixel_motion.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api, scenes  # noqa: E402

WARM, RUNS = 2, 11
W, H = 1920, 1080


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    s, p = scenes.heightfield(W, H, 1, 2, n=256)
    p = dict(p, eye=(0.0, 9.0, 3.0), target=(0.0, 0.6, 0.0))     # from above: the height field fills most of the frame
    mesh = 1
    base = np.ascontiguousarray(s.meshes[mesh].positions, np.float32)
    sets = [np.ascontiguousarray(base * np.float32(1.0 + 0.03 * (k + 1))) for k in range(2)]
    scene = api.DeviceScene(s, device=0)
    acc, plain = api.TemporalAccumulator(W, H, device=0), api.TemporalAccumulator(W, H, device=0)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    frame, variance = f32(H, W, 4), f32(H, W)
    feats = dict(position=f32(H, W, 3), normal=f32(H, W, 3), depth=f32(H, W), coverage=f32(H, W),
                 ids=torch.empty((H, W, 4), dtype=torch.int32, device="cuda"))
    records, out, out_var = f32(H, W, 8), f32(H, W, 4), f32(H, W)
    stream = torch.cuda.current_stream().cuda_stream
    times = {k: ([], []) for k in ("keep_previous", "update_meshes", "pixel_motion", "accumulate", "accumulate, no motion")}
    update_device, moved = [], []

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record()
        e1.synchronize()
        times[name][0].append(e0.elapsed_time(e1))
        times[name][1].append(wall)

    for k in range(WARM + RUNS + 1):
        if k:
            timed("keep_previous", lambda: scene.keep_previous(stream))
            timed("update_meshes", lambda: scene.update_meshes({mesh: sets[k % 2]}, stream=stream))
            update_device.append(scene.last_update["ms_device"])
        scene.render_moments_into(frame, feats, {"variance": variance}, p, stream=stream)
        if k:
            timed("pixel_motion", lambda: scene.pixel_motion_into(records, feats, stream=stream))
            moved.append(float((records.view(torch.int32)[..., 3] == 1).float().mean()))
            timed("accumulate", lambda: acc.accumulate_into(out, out_var, None, p, frame, variance, feats, demodulate=False, stream=stream,
                                                            pixel_motion=records))
        else:
            acc.accumulate_into(out, out_var, None, p, frame, variance, feats, demodulate=False, stream=stream)
        timed("accumulate, no motion", lambda: plain.accumulate_into(out, out_var, None, p, frame, variance, feats, demodulate=False, stream=stream))
    med = lambda v: statistics.median(v[-RUNS:])
    tris = sum(len(m.faces) for m in s.meshes)
    lines = [f"# tools/pixel_motion_trace.py: {W} x {H}, scenes.heightfield(n=256), {tris} tris, mesh {mesh} deforms ({len(s.meshes[mesh].faces)} tris, "
             f"{len(base)} vertices); median of {RUNS} frames after {WARM} warm-up frames; device events around the call | wall time of the call",
             f"# pixels whose record is `moved`: {statistics.median(moved[-RUNS:]):.3f} of the frame"]
    for name, (dev, wall) in times.items():
        lines.append(f"{name:<24} device {med(dev):8.3f} ms | wall {med(wall):8.3f} ms   (min {min(dev[-RUNS:]):.3f}, max {max(dev[-RUNS:]):.3f})")
    lines.append(f"{'update_meshes (stats)':<24} device {med(update_device):8.3f} ms   (profiles/mesh_update.txt: 9.866 ms with normals and tangents passed)")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    acc.close()
    plain.close()
    scene.close()


if __name__ == "__main__":
    main()
