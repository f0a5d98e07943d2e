"""Wall time of yart_hip_scene_update_textures against re-creating the device scene (profiles/texture_update.txt).

Three rows on scenes.material_test(tex=1024): (a) its bundled 1024^2 base-colour map (the floor's: a member of a base + normal +
metal-rough bundle and of a base + metal-rough bundle; all alpha 255, so a reduction and no chain); (b) its `t_leaf` map, the alpha
card's, with new cut-out texels — the flag stays, no chain; (c) the same map between the cut-out and all-opaque texels — the flag flips
every call, and the chain runs over the scene's main mesh. For each: yart_hip_scene_destroy + yart_hip_scene_create of the same
description (the C calls alone: the description is marshalled once; what a caller without the update has to do per frame), and the
update from host pixels, two states in turn — one warm-up, then the median of 5 runs each, the call's own statistics (ms_total: wall
time of the call, which ends in a synchronise; ms_device: between the events around its stream work) — and once more from device
pixels (a torch uint8 tensor: what a decoder or a procedural map hands over).

    python tools/texture_update_trace.py [--out profiles/texture_update.txt] [--tex 1024]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yart_amd import api, scenes  # noqa: E402
from update_trace_common import recreate_ms, scene_over, update_stats  # noqa: E402

def measure(name, s, updates, out):
    """updates: two {texture: uint8 array} taken in turn"""
    import torch
    L = api.lib()
    create, h = recreate_ms(s)
    scene = scene_over(h)
    rows = []
    on_device = [{t: torch.from_numpy(np.ascontiguousarray(px)).to("cuda:0") for t, px in u.items()} for u in updates]
    torch.cuda.synchronize()
    for tag, args in (("host pixels", updates), ("device pixels", on_device)):
        total, device, launches = update_stats(lambda k: scene.update_textures(args[k % 2]) or scene.last_update)
        rows.append((tag, statistics.median(total[1:]), statistics.median(device[1:]), sorted(set(launches[1:])), total[0]))
    L.yart_hip_scene_destroy(h)
    scene._h = C.c_void_p()
    tris = sum(len(x.faces) for x in s.meshes)
    mb = sum(px.nbytes for px in updates[0].values()) / 1e6
    line = f"{name:<44} {tris:>6} tris, {mb:5.2f} MB of texels passed | destroy+create {create:>8.3f} ms"
    for tag, total, device, launches, first in rows:
        line += (f" | update_textures, {tag}: total {total:.3f} ms, device {device:.3f} ms, launches {'/'.join(str(v) for v in launches)} "
                 f"(first call {first:.3f} ms), {'FASTER' if total < create else 'NOT FASTER'} than re-creation ({create / total:.1f}x)")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tex", type=int, default=1024)
    a = ap.parse_args()
    import torch                                              # (first: the process then has one HIP runtime, torch's and the library's)
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda").cpu()
    out = ["# tools/texture_update_trace.py: median of 5 runs after one warm-up; wall time of the C calls, each ending in a synchronise.",
           "# Footprint records: k_tex_quads once per place (the texture's own array, each bundle that holds it) — the per-member form is",
           "# the one kept; a fused kernel that rewrites a bundle's whole 64-byte records was not built or measured."]
    s, _ = scenes.material_test(tex=a.tex)
    t_base, t_leaf = s.materials[0].tex_base, next(m.tex_base for m in s.materials if m.tex_base >= 0 and m.tex_mr < 0)
    assert t_base != t_leaf and (s.textures[t_leaf].data[..., 3] < 255).any() and not (s.textures[t_base].data[..., 3] < 255).any()
    base0 = s.textures[t_base].data
    base1 = scenes.tex_base_color(a.tex, 11, (0.2, 0.3, 0.7), (0.9, 0.9, 0.5)).data
    leaf0 = s.textures[t_leaf].data
    leaf1 = scenes.tex_base_color(a.tex, 12, (0.4, 0.3, 0.1), (0.7, 0.6, 0.2), alpha=scenes.tex_alpha_leaves(a.tex, 13)).data
    opaque = leaf0.copy()
    opaque[..., 3] = 255
    assert (leaf1[..., 3] < 255).any()
    measure(f"(a) material_test(tex={a.tex}): bundled base map", s, [{t_base: base1}, {t_base: base0}], out)
    measure(f"(b) material_test(tex={a.tex}): t_leaf, no flip", s, [{t_leaf: leaf1}, {t_leaf: leaf0}], out)
    measure(f"(c) material_test(tex={a.tex}): t_leaf, flag flips", s, [{t_leaf: opaque}, {t_leaf: leaf0}], out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
