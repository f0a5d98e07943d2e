"""Russian roulette decided in the shade kernel (csrc/wavefront.hpp: wfRouletteTentative, wfShadowCommitGeneral).

The reference draws a path's roulette after the bounce's shadow ray (mis-integrator.cpp:96-102), whose alpha tests may consume
sampler dimensions first. k_wf_shade takes the decision before the shadow stage, at the dimension the shadow walk starts with;
only the general shadow kernels have a sampler, so only they can find the walk's dimension moved, and they take the decision
again and repair one that flipped. Four scenes, one per way through that code, each with and without path-state compaction
(the pending flag and the unscaled throughput must survive k_wf_compact's copy):

  deep_tree         every alpha candidate has 0 < alpha < 1: every handed-over shadow ray draws, decisions flip both ways
  alpha_instances   alpha candidates of alpha 0 and 1, and thin glass: hand-overs inside transformed nodes
  cornell           no alpha at all: every tentative decision is final
  material_test     glass and clearcoat panels: throughputs >= 1, for which no roulette applies at any depth

Every frame is compared on bits with the CPU oracle and with the megakernel (one path loop, the reference's order of draws);
per-pixel ray counts and the paths that enter each bounce are compared with the pipeline that traces every ray with the
general kernels. The counting library says how many decisions were reversed."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ORACLE_BIN, bit_identical_or_drift

pytestmark = pytest.mark.gpu

MEGAKERNEL, GENERAL_TRACE, NO_REFILL, NO_COMPACTION = 1, 4, 16, 32


def _case(name):
    from yart_amd import scenes
    if name == "deep_tree":
        return scenes.deep_tree(6, alpha_levels=(1, 3), width=48, height=48, spp=8, bounces=6)
    if name == "alpha_instances":
        return scenes.alpha_instances(96, 96, 4, 5)
    if name == "cornell":
        return scenes.cornell(64, 64, 16, 8)
    if name == "material_test":
        return scenes.material_test(64, 64, 8, 6)
    raise KeyError(name)


CASES = ["deep_tree", "alpha_instances", "cornell", "material_test"]


@pytest.fixture(scope="module")
def api(built):
    from yart_amd import api
    assert api.lib().yart_hip_device_count() > 0, "no HIP device: the GPU tests need the real kernels"
    return api


@pytest.fixture(scope="module")
def references(api, oracle_bin, tmp_path_factory):
    """Per case, computed once and only read afterwards: the scene, its parameters, the oracle's frame, and the megakernel's
    frame with its per-pixel and total ray counts."""
    from yart_amd import scenes
    cache = {}

    def get(name):
        if name not in cache:
            s, p = _case(name)
            d = tmp_path_factory.mktemp(name)
            sp, pp, out = d / "s.yscn", d / "s.txt", d / "s.f32"
            s.save(sp); scenes.write_params(pp, p)
            subprocess.run([ORACLE_BIN, "render", str(sp), str(pp), str(out)], check=True, stdout=subprocess.DEVNULL)
            ds = api.DeviceScene(s, device=0)
            mega, aov, st = ds.render_aovs(p, aovs=("rays",), flags=MEGAKERNEL)
            ds.close()
            oracle = np.fromfile(out, np.float32).reshape(mega.shape)
            for a in (oracle, mega, aov["rays"]):
                a.setflags(write=False)
            cache[name] = dict(scene=s, params=p, oracle=oracle, mega=mega, mega_rays=aov["rays"], mega_total=st["rays"])
        return cache[name]
    return get


@pytest.mark.parametrize("compaction", ["compact", "no_compact"])
@pytest.mark.parametrize("name", CASES)
def test_frames_rays_and_paths(api, references, name, compaction):
    """The default pipeline, the one-ray-per-lane lean kernels and the general-only pipeline: the oracle's and the megakernel's
    frame bit for bit, the megakernel's ray count per pixel, and one count of paths per bounce among the three."""
    r = references(name)
    extra = NO_COMPACTION if compaction == "no_compact" else 0
    ds = api.DeviceScene(r["scene"], device=0)
    got = {}
    for tag, flags in (("general", GENERAL_TRACE), ("default", 0), ("no_refill", NO_REFILL)):
        img, aov, st = ds.render_aovs(r["params"], aovs=("rays",), flags=flags | extra)
        got[tag] = (aov["rays"], st)
        bit_identical_or_drift(img, r["oracle"], f"{name}/{tag}/{compaction} vs oracle")
        assert np.array_equal(img.view(np.uint32), r["mega"].view(np.uint32)), f"{name}/{tag}/{compaction} vs megakernel"
    ds.close()
    gen_rays, gen_st = got["general"]
    assert np.array_equal(gen_rays, r["mega_rays"]) and gen_st["rays"] == r["mega_total"]
    depth = r["params"]["depth"]
    print(f"{name}/{compaction}: paths_at_bounce {list(gen_st['paths_at_bounce'][:depth])}")
    assert gen_st["paths_at_bounce"][0] > 0 and gen_st["paths_at_bounce"][min(2, depth - 1)] > 0
    for tag in ("default", "no_refill"):
        rays, st = got[tag]
        assert np.array_equal(rays, gen_rays), f"{name}/{tag}/{compaction}: per-pixel ray counts"
        assert st["rays"] == gen_st["rays"], f"{name}/{tag}/{compaction}: rays"
        assert list(st["paths_at_bounce"]) == list(gen_st["paths_at_bounce"]), f"{name}/{tag}/{compaction}: paths_at_bounce"


@pytest.mark.parametrize("name", CASES)
def test_reversed_decisions(api, references, name):
    """The counting library (debug counters 10 / 11: tentative decisions reversed dead -> alive / alive -> dead, 30: shadow
    rays handed to the general kernel) renders the same frame and reports what the scene is there for. deep_tree (48x48, 8 spp,
    6 bounces, seed 3): at least one decision reversed in each direction; cornell: no hand-over, so none; the other two: printed.
    An entry of a path reversed to dead is shaded no more: shade_entries and rays equal the general-only pipeline's."""
    r = references(name)
    ds = api.DeviceScene(r["scene"], device=0, instrumented=True)
    seen = {}
    for tag, flags in (("default", 0), ("default/no_compact", NO_COMPACTION), ("general", GENERAL_TRACE)):
        img, st = ds.render(r["params"], flags=flags)
        c = ds.debug_counters()
        assert np.array_equal(img.view(np.uint32), r["oracle"].view(np.uint32)), f"{name}/{tag} (counting library) vs oracle"
        seen[tag] = dict(alive=int(c[10]), dead=int(c[11]), handed=int(c[30]), rays=st["rays"], hits=st["shaded_hits"],
                         entries=st["shade_entries"])
        print(f"{name}/{tag}: {seen[tag]}")
    ds.close()
    for tag in ("default", "default/no_compact"):
        for key in ("rays", "hits", "entries"):
            assert seen[tag][key] == seen["general"][key], (name, tag, key)
    assert seen["default"]["rays"] == r["mega_total"]
    assert seen["default/no_compact"] == seen["default"]
    if name == "deep_tree":
        assert seen["default"]["handed"] > 0
        for tag in seen:
            assert seen[tag]["alive"] >= 1 and seen[tag]["dead"] >= 1, (tag, seen[tag])
        # a ray the lean kernel commits met no alpha candidate, so the general kernel draws nothing for it either: the walks that
        # draw, and with them the reversals, are the same whichever kernel does them
        assert (seen["general"]["alive"], seen["general"]["dead"]) == (seen["default"]["alive"], seen["default"]["dead"])
    if name == "cornell":
        for tag in seen:
            assert seen[tag]["alive"] == 0 and seen[tag]["dead"] == 0 and seen[tag]["handed"] == 0, (tag, seen[tag])
