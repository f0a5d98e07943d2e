"""One process, no counters: five iterations of the à-trous filter with all three guides, demodulated, at 1920 x 1080 and at
3840 x 2160 on random device tensors (api.denoise_into), three calls per size; with --var the variance-guided form
(api.denoise_var_into) with a random non-negative variance tensor. Meant to run under a kernel trace:

  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d profile_out -o denoise -- python tools/denoise_trace.py [--var]

(the *_kernel_stats.csv of that run is profiles/denoise_kernel_stats.csv, with --var profiles/denoise_var_kernel_stats.csv).
Prints the wall time per call as well."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api  # noqa: E402

VAR = "--var" in sys.argv[1:]
for w, h in ((1920, 1080), (3840, 2160)):
    g = torch.Generator(device="cuda").manual_seed(w)
    frame = torch.rand((h, w, 4), device="cuda", generator=g) * 4
    guides = {"albedo": torch.rand((h, w, 3), device="cuda", generator=g),
              "normal": torch.nn.functional.normalize(torch.randn((h, w, 3), device="cuda", generator=g), dim=-1).contiguous(),
              "depth": torch.rand((h, w), device="cuda", generator=g) * 50 + 0.1}
    variance = torch.rand((h, w), device="cuda", generator=g) * 2 if VAR else None
    out = torch.empty_like(frame)
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if VAR:
            api.denoise_var_into(out, frame, variance, guides, iterations=5, demodulate=True)
        else:
            api.denoise_into(out, frame, guides, iterations=5, demodulate=True)
        print(f"{w}x{h} call {rep}: {(time.perf_counter() - t0) * 1e3:.2f} ms (allocation of the scratch included)", flush=True)
