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

is profiles/temporal_moments_kernel_stats.csv; the wall times printed tell the first frame's pass 2 from the steady one's."""
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
MOMENTS = ap.parse_args().moments

for w, h in ((1920, 1080),) if MOMENTS else ((1920, 1080), (3840, 2160)):
    g = torch.Generator(device="cuda").manual_seed(w)
    acc = api.TemporalAccumulator(w, h, device=torch.cuda.current_device(), moments=MOMENTS)
    out, out_var = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w), device="cuda")
    length = torch.empty((h, w), dtype=torch.int32, device="cuda")
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
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.accumulate_into(out, out_var, length, cam, frame, var, aovs, demodulate=True)
        if MOMENTS:
            print(f"  pixels at or past min_moment_history {(length >= acc.params['min_moment_history']).float().mean().item():.3f}; "
                  f"pixels with a variance {(out_var > 0).float().mean().item():.3f}")
        print(f"{w}x{h} frame {k}: {(time.perf_counter() - t0) * 1e3:.2f} ms (frame 0: allocation of the history included); "
              f"pixels with a history {(length > 1).float().mean().item():.3f}", flush=True)
    acc.close()
