"""One process, no counters: three frames of the temporal accumulator (demodulated, all outputs) at 1920 x 1080 and at
3840 x 2160 on synthetic device tensors (api.TemporalAccumulator.accumulate_into): a plane seen by a camera that pans a few
pixels per frame, so that the second and third frame read their four taps. Meant to run under a kernel trace:

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profile_out -o temporal -- python tools/temporal_trace.py

(the *_kernel_stats.csv of that run is profiles/temporal_kernel_stats.csv). Prints the wall time per call as well.

--moments: the moments form (k_tp_accumulate<true> + k_tp_spatial_variance) at the default min_moment_history, at 1920 x 1080 only,
with an input variance of 0 (1 spp): frame 0 is a first frame, where every pixel is short and walks its 7 x 7 window, then six more
frames, of which those from the fourth on are steady (every pixel long: pass 2 returns after its own two loads). The
*_kernel_stats.csv of

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profile_out -o temporal_moments -- python tools/temporal_trace.py --moments

is profiles/temporal_moments_kernel_stats.csv; the wall times printed tell the first frame's pass 2 from the steady one's.

--motion: the plain form at both sizes with a per-node motion (k_tp_accumulate<false, true>) next to the same frames without one
(k_tp_accumulate<false, false>, the kernel from before there was a motion) on a second accumulator, same inputs: the left half of
the image is node 0, which slides 3 pixels a frame within the plane (a moving record: six 16-byte loads per lane), the right half
node 1 with a static record (one load); 64 records. The *_kernel_stats.csv of

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profile_out -o temporal_motion -- python tools/temporal_trace.py --motion

is profiles/temporal_motion_kernel_stats.csv."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api  # noqa: E402
from yart_amd.temporal import camera_basis  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--moments", action="store_true")
ap.add_argument("--motion", action="store_true")
MOMENTS, MOTION = ap.parse_args().moments, ap.parse_args().motion
assert not (MOMENTS and MOTION)

for w, h in ((1920, 1080),) if MOMENTS else ((1920, 1080), (3840, 2160)):
    g = torch.Generator(device="cuda").manual_seed(w)
    acc = api.TemporalAccumulator(w, h, device=torch.cuda.current_device(), moments=MOMENTS)
    out, out_var = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w), device="cuda")
    length = torch.empty((h, w), dtype=torch.int32, device="cuda")
    still = api.TemporalAccumulator(w, h, device=torch.cuda.current_device()) if MOTION else None
    for k in range(7 if MOMENTS else 3):
        cam = dict(size=(w, h), focal=35.0, sensor=(36.0, 24.0), eye=(0.01 * k, 0.0, 5.0), target=(0.01 * k, 0.0, 0.0), up=(0.0, 1.0, 0.0))
        b = {name: torch.from_numpy(np.asarray(v)).cuda() for name, v in camera_basis(cam).items()}
        ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                                indexing="ij")
        pos = (b["top_left"] + xs[..., None] * b["dU"] + ys[..., None] * b["dV"]).contiguous()       # the focus plane z = 0 itself
        aovs = {"position": pos, "normal": torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(h, w, 3).contiguous(),
                "depth": (pos - b["position"]).norm(dim=-1).contiguous(), "coverage": torch.ones((h, w), device="cuda"),
                "ids": torch.zeros((h, w, 4), dtype=torch.int32, device="cuda"),
                "albedo": torch.rand((h, w, 3), device="cuda", generator=g)}
        frame = torch.rand((h, w, 4), device="cuda", generator=g) * 4
        var = torch.zeros((h, w), device="cuda") if MOMENTS else torch.rand((h, w), device="cuda", generator=g)
        motion = None
        if MOTION:
            aovs["ids"][:, w // 2:, 0] = 1
            motion = np.zeros((64, 24), np.float32)
            motion[0, [0, 5, 10, 12, 17, 22]] = 1.0                                                   # M, Nm: the identity ...
            motion[0, 3] = -3.0 * float(np.linalg.norm(camera_basis(cam)["dU"]))                      # ... and 3 pixels back in x
            motion.view(np.uint32)[0, 15] = 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            still.accumulate_into(out, out_var, length, cam, frame, var, aovs, demodulate=True)
            print(f"{w}x{h} frame {k}, no motion: {(time.perf_counter() - t0) * 1e3:.2f} ms; "
                  f"pixels with a history {(length > 1).float().mean().item():.3f}", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.accumulate_into(out, out_var, length, cam, frame, var, aovs, demodulate=True, motion=motion)
        if MOMENTS:
            print(f"  pixels at or past min_moment_history {(length >= acc.params['min_moment_history']).float().mean().item():.3f}; "
                  f"pixels with a variance {(out_var > 0).float().mean().item():.3f}")
        print(f"{w}x{h} frame {k}: {(time.perf_counter() - t0) * 1e3:.2f} ms (frame 0: allocation of the history included); "
              f"pixels with a history {(length > 1).float().mean().item():.3f}", flush=True)
    acc.close()
    if still is not None:
        still.close()
