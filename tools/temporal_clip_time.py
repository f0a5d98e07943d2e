"""Times yart_hip_temporal_accumulate[_moments]_device at 1920 x 1080 with and without a clip (profiles/temporal_clip.txt).

  python tools/temporal_clip_time.py [--parent PATH/libyart_hip.so] [--out profiles/temporal_clip_times.txt]

Plain and moments form, no clip / radius 1 / radius 3 at the default gamma, out of place and in place (the staging copy), on torch
device tensors; --parent: another build of the library (the parent commit's) on the same unclipped call, its windows alternating
with this build's. Inputs: a static camera on one plane, uniform noise: every pixel has a counting tap set, so every pixel runs
the clip. A host clock around calls that return after completion on their stream."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yart_amd import api, temporal  # noqa: E402
from tests import test_temporal as tt  # noqa: E402

W, H = 1920, 1080
REPEATS, CALLS = 7, 40


def frames(n=2):
    rng = np.random.RandomState(3)
    cam = tt.base_camera(W, H)
    _, plane, _, p = tt.see(cam, 1e6)
    depth = np.linalg.norm(p - np.array(cam["eye"]), axis=-1).astype(np.float32)
    nrm = (np.where(plane[..., None] == 2, -1.0, 1.0) * np.array([0.0, 0.0, 1.0])).astype(np.float32)
    ids = np.zeros((H, W, 4), np.int32)
    ids[..., 0] = plane
    out = []
    for _ in range(n):
        rgba = np.ones((H, W, 4), np.float32)
        rgba[..., :3] = rng.uniform(0.2, 2.0, (H, W, 3))
        out.append(dict(rgba=rgba, variance=rng.uniform(0, 1, (H, W)).astype(np.float32), position=p.astype(np.float32), normal=nrm,
                        depth=depth, coverage=np.ones((H, W), np.float32), ids=ids, albedo=rng.uniform(0.1, 1, (H, W, 3)).astype(np.float32)))
    return cam, out


class Raw:
    """the accumulate entries of one library through ctypes (the parent's has no set_clip)"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.h = {}

    def handle(self, moments, clip):
        key = (moments, clip)
        if key not in self.h:
            h = C.c_void_p()
            assert self.L.yart_hip_temporal_create(W, H, 0, C.byref(h)) == 0
            if clip:
                tc = api.TemporalClip(C.sizeof(api.TemporalClip), clip[0], clip[1])
                self.L.yart_hip_temporal_set_clip.argtypes = [C.c_void_p, C.POINTER(api.TemporalClip)]
                assert self.L.yart_hip_temporal_set_clip(h, C.byref(tc)) == 0
            self.h[key] = h
        return self.h[key]

    def call(self, moments, clip, cam, t, out, var, ln, in_place):
        fn = self.L.yart_hip_temporal_accumulate_moments_device if moments else self.L.yart_hip_temporal_accumulate_device
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ab = api.AovBuffers()
        ab.struct_size = C.sizeof(api.AovBuffers)
        for name in api.TEMPORAL_AOVS + ("albedo",):
            ab.mask |= api.AOVS[name][0]
            setattr(ab, name, C.c_void_p(t[name].data_ptr()))
        tp = (api.make_temporal_moment_params if moments else api.make_temporal_params)(demodulate=True)
        o = t["rgba"] if in_place else out
        v = t["variance"] if in_place else var
        r = fn(self.h[(moments, clip)], C.byref(cam), t["rgba"].data_ptr(), t["variance"].data_ptr(), C.byref(ab), C.byref(tp),
               o.data_ptr(), v.data_ptr(), ln.data_ptr(), None)
        assert r == 0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_clip_times.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    cam, fr = frames()
    camd = api.make_camera(cam)
    t = [{k: torch.from_numpy(v).cuda() for k, v in f.items()} for f in fr]
    out, var = torch.zeros_like(t[0]["rgba"]), torch.zeros_like(t[0]["variance"])
    ln = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    libs = {"this": Raw(api.LIB_PATH)}
    gamma = temporal.DEFAULT_CLIP_GAMMA
    cases = [("this", None), ("this", (1, gamma)), ("this", (3, gamma))]
    if args.parent:
        libs["parent"] = Raw(args.parent)
        cases.insert(0, ("parent", None))
    lines = [f"accumulate_device at {W} x {H}, demodulated, default parameters; every pixel has a counting tap set",
             f"ms per call: median (min .. max) over {REPEATS} windows of {CALLS} calls, host clock around calls that return after completion;",
             "the cases of a row alternate window by window"]
    for moments in (False, True):
        for in_place in (False, True):
            times = {c: [] for c in cases}
            for lib, clip in cases:
                libs[lib].handle(moments, clip)
                for k in range(4):                            # warm-up: code objects, the history and staging allocations
                    libs[lib].call(moments, clip, camd, t[k % 2], out, var, ln, in_place)
            for _ in range(REPEATS):
                for lib, clip in cases:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(CALLS):
                        libs[lib].call(moments, clip, camd, t[k % 2], out, var, ln, in_place)
                    torch.cuda.synchronize()
                    times[(lib, clip)].append((time.perf_counter() - t0) / CALLS * 1e3)
            for (lib, clip), v in times.items():
                v = sorted(v)
                lines.append(f"{'moments' if moments else 'plain  '} {'in place    ' if in_place else 'out of place'} {lib:<6} "
                             f"clip {str(clip):<10} {v[len(v) // 2]:.4f} ({v[0]:.4f} .. {v[-1]:.4f})")
                print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
