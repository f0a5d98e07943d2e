"""Wall time of yart_hip_scene_update_lighting against re-creating the device scene (profiles/lighting_update.txt).

Three rows: (a) scenes.material_test(tex=1024) — materials and lights only, nothing is launched; (b) the geometry of
scenes.sponza_class at a small `detail` and small material textures under its 2048^2 sky, the sky's texels replaced — upload, footprint
records and the image light's tables rebuilt on the device; (c) the same under a 512^2 sky. For each: yart_hip_scene_destroy +
yart_hip_scene_create of the same description (the C calls alone: the description is marshalled once; what a caller without the
update has to do per frame), and the update, two states in turn — one warm-up, then the median of 5 runs each, the call's own
statistics (ms_total: wall time of the call, which ends in a synchronise; ms_device: between the events around its stream work). For
the image rows also, separately: the host's sequential texel sum (yart_hip_probe_texel_sum: the library takes it while the device
works) and a pageable host-to-device copy of the same bytes (torch), the two parts of the call that are not kernels.

    python tools/lighting_update_trace.py [--out profiles/lighting_update.txt] [--detail 0.1]"""
import argparse
import copy
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import median_ms, recreate_ms, scene_over, update_stats  # noqa: E402

def measure(name, s, updates, out):
    """updates: two argument sets (materials, lights, images) taken in turn"""
    L = api.lib()
    create, h = recreate_ms(s)
    scene = scene_over(h)
    total, device, launches = update_stats(lambda k: scene.update_lighting(**updates[k % 2]) or scene.last_update)
    L.yart_hip_scene_destroy(h)
    scene._h = C.c_void_p()
    tris = sum(len(x.faces) for x in s.meshes)
    texels = sum(t.width * t.height for t in s.textures)
    upd_total = statistics.median(total[1:])
    line = (f"{name:<34} {tris:>7} tris, {texels / 1e6:6.2f} M texels, passed: {'+'.join(sorted(updates[0]))} | destroy+create {create:>9.3f} ms | "
            f"update_lighting: total {upd_total:.3f} ms, device {statistics.median(device[1:]):.3f} ms, {launches[-1]} launches (first call {total[0]:.3f} ms)"
            f" | {'FASTER' if upd_total < create else 'NOT FASTER'} than re-creation ({create / upd_total:.1f}x)")
    images = updates[0].get("images")
    if images:
        import torch
        img = np.ascontiguousarray(next(iter(images.values())), np.float32)
        sum3 = np.zeros(3, np.float32)
        host_sum = median_ms(lambda: L.yart_hip_probe_texel_sum(img.ctypes.data_as(C.c_void_p), img.shape[0] * img.shape[1], sum3.ctypes.data_as(C.c_void_p)))
        dst = torch.empty(img.shape, dtype=torch.float32, device="cuda:0")
        src = torch.from_numpy(img)

        def upload():
            dst.copy_(src)
            torch.cuda.synchronize()
        line += f" | alone: host texel sum {host_sum:.3f} ms, pageable upload of {img.nbytes / 1e6:.1f} MB {median_ms(upload):.3f} ms"
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--detail", type=float, default=0.1)
    a = ap.parse_args()
    import torch                                              # (first: the process then has one HIP runtime, torch's and the library's)
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()
    out = ["# tools/lighting_update_trace.py: median of 5 runs after one warm-up; wall time of the C calls, each ending in a synchronise"]
    s, _ = scenes.material_test(tex=1024)
    s1 = copy.deepcopy(s)
    for m in s1.materials:
        m.base = tuple(0.5 * v for v in m.base); m.roughness = min(1.0, m.roughness + 0.1)
        m.emission = tuple(0.25 * v for v in m.emission)
    for l in s1.lights:
        l.emission = tuple(0.25 * v for v in l.emission)
    measure("(a) material_test(tex=1024)", s, [dict(materials=s1.materials, lights=s1.lights), dict(materials=s.materials, lights=s.lights)], out)
    for tag, sky in (("(b)", 2048), ("(c)", 512)):
        s, _ = scenes.sponza_class(detail=a.detail, tex=128, sky=sky)
        tex = next(l.texture for l in s.lights if l.type == 2)
        other = scenes.sky_octahedral(sky, sun_dir=(-0.6, 0.3, 0.5)).data
        measure(f"{tag} sponza_class(detail={a.detail}, sky={sky})", s, [dict(images={tex: other}), dict(images={tex: s.textures[tex].data})], out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
