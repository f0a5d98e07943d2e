"""Every kernel of the two product libraries is emitted in exactly one translation unit.

The libraries are five units each (csrc/Makefile); a kernel that is not a template is emitted by every unit whose source
holds its definition, and only one unit launches it. The code objects' symbol tables name every kernel's descriptor
(NAME.kd), so the bytes of the library tell how many code objects define a kernel: no tool and no compile needed."""
import collections
import os
import re

import pytest

from tests.conftest import ROOT

KD = re.compile(rb"(_Z\w*k_\w+)\.kd\x00")      # e.g. _ZN12_GLOBAL__N_113k_wf_generateENS_6WfArgsE.kd


@pytest.mark.parametrize("name", ["libyart_hip.so", "libyart_hip_count.so"])
def test_every_kernel_is_in_one_unit(built, name):
    blob = open(os.path.join(ROOT, "yart_amd", name), "rb").read()
    counts = collections.Counter(m.group(1).decode() for m in KD.finditer(blob))
    # an empty or compressed fat binary must fail, not pass: kernels of unit 0, of the streaming passes and of units 4 and 1
    for needle in ("12k_gmon_blendE", "13k_wf_generateE", "13k_wf_rouletteE", "10k_wf_shadeIL", "16k_wf_extend_leanIL", "15k_probe_shadingE"):
        assert any(needle in k for k in counts), f"{name}: no kernel descriptor matches {needle}"
    gmon = [k for k in counts if "12k_gmon_blendE" in k]
    assert len(gmon) == 1, gmon
    once = counts[gmon[0]]                     # occurrences of a name that one code object defines (its symbol and string tables)
    print(f"{name}: {len(counts)} kernels, {once} occurrences of k_gmon_blend's descriptor name")
    more = {k: n for k, n in counts.items() if n != once}
    assert not more, f"{name}: kernels that do not occur {once} times (one code object each): {more}"
