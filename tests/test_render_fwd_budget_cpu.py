"""The register budget of the one-wave-per-tile blend forward, read from the code object's metadata (no GPU): render_fwd.hip is
compiled for gfx950 to assembly with the flags of luciddreamer_amd/build.py, the way tools/kernel_compare.py does, and every
k_render_fwd_tile instantiation must fit amdgpu_num_vgpr(64) -- 8 waves per SIMD, all 8160 tiles of a 1080p view resident at once
-- without a private segment (no scratch), in 3 KB of LDS.  Only kernel descriptors are read.

Measured on this source, <STRICT, DEPTH, COLOR>: VGPRs / private segment bytes
    <0,0,0> 64 / 0   <1,0,0> 61 / 0      colour-free (two copies of the rounds in one kernel: 63 -> 64 and 60 -> 61 registers)
    <0,0,1> 63 / 0   <1,0,1> 60 / 0      colour
    <0,1,1> 64 / 0   <1,1,1> 64 / 0      colour + depth
<0,1,1> used to spill three dwords (64 / 12 B, profiles/step_invariants_ab.txt); render_fwd_tile's TIGHT measures removed them.
"""
import os
import re
import subprocess

import pytest

from luciddreamer_amd import build

CASES = [(st, dp, cl) for st in (0, 1) for dp, cl in ((0, 0), (0, 1), (1, 1))]


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    """{(STRICT, DEPTH, COLOR): {descriptor field: int}} of the k_render_fwd_tile kernels."""
    tmp = tmp_path_factory.mktemp("render_fwd_asm")
    (tmp / "lr_src_hash.h").write_text('#define LR_SRC_HASH "budget"\n')
    out = tmp / "render_fwd.s"
    flags = [f for f in build.COMMON_FLAGS if f != build.INCLUDE and f not in ("-I", "-fPIC")]
    cmd = [build.hipcc(), "-S", "--cuda-device-only", os.path.join(build.CSRC, "render_fwd.hip"), "-o", str(out)] + flags + \
          ["-I", build.INCLUDE, "-I", str(tmp)] + build.SOURCES["render_fwd.hip"]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    found = {}
    for name, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", out.read_text(), flags=re.M | re.S):
        m = re.search(r"17k_render_fwd_tileILb([01])ELb([01])ELb([01])EE", name)
        if m:
            found[tuple(int(x) for x in m.groups())] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", body, flags=re.M)}
    return found


def test_the_three_channel_sets_and_no_fourth(descriptors):
    assert sorted(descriptors) == sorted(CASES)


@pytest.mark.parametrize("strict,depth,color", CASES)
def test_tile_forward_fits_its_budget(descriptors, strict, depth, color):
    """At most 64 VGPRs, no private segment, 3 KB of LDS."""
    d = descriptors[(strict, depth, color)]
    print(f"k_render_fwd_tile<{strict},{depth},{color}>: next_free_vgpr {d['next_free_vgpr']}, private segment "
          f"{d['private_segment_fixed_size']} B, LDS {d['group_segment_fixed_size']} B")
    assert d["next_free_vgpr"] <= 64
    assert d["private_segment_fixed_size"] == 0
    assert d["group_segment_fixed_size"] <= 3072
