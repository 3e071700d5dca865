"""The register budget of the fused step kernel (render_bwd.hip k_render_bwd_tile_step: a tile's blend forward and backward in one
wave), read from the code object's metadata (no GPU), as tests/test_render_fwd_budget_cpu.py does for the tile forward:
render_bwd.hip is compiled for gfx950 to assembly with the flags of luciddreamer_amd/build.py, and both STRICT instantiations
must fit amdgpu_num_vgpr(64) -- 8 waves per SIMD, all 8160 tiles of a 1080p view resident at once -- without a private segment
(no scratch), within the 5120 bytes of LDS that 32 waves per CU leave each of them (160 KB / 32).  Only kernel descriptors are read.

Measured on this source, <STRICT>: VGPRs / private segment bytes / LDS bytes
    <0> 64 / 0 / 5064      <1> 64 / 0 / 5064
(5056 bytes shared by the two halves -- the forward's three staging planes lie inside the backward's -- and 8 for the address of
the argument segment, which waits in LDS while the forward half runs.)
"""
import os
import re
import subprocess

import pytest

from luciddreamer_amd import build


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    """{STRICT: {descriptor field: int}} of the k_render_bwd_tile_step kernels."""
    tmp = tmp_path_factory.mktemp("render_bwd_asm")
    (tmp / "lr_src_hash.h").write_text('#define LR_SRC_HASH "budget"\n')
    out = tmp / "render_bwd.s"
    flags = [f for f in build.COMMON_FLAGS if f != build.INCLUDE and f not in ("-I", "-fPIC")]
    cmd = [build.hipcc(), "-S", "--cuda-device-only", os.path.join(build.CSRC, "render_bwd.hip"), "-o", str(out)] + flags + \
          ["-I", build.INCLUDE, "-I", str(tmp)] + build.SOURCES["render_bwd.hip"]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    found = {}
    for name, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", out.read_text(), flags=re.M | re.S):
        m = re.search(r"22k_render_bwd_tile_stepILb([01])EE", name)
        if m:
            found[int(m.group(1))] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)\s*$", body, flags=re.M)}
    return found


def test_both_instantiations_and_no_third(descriptors):
    assert sorted(descriptors) == [0, 1]


@pytest.mark.parametrize("strict", [0, 1])
def test_fused_step_kernel_fits_its_budget(descriptors, strict):
    """At most 64 VGPRs, no private segment, at most 5120 bytes of LDS."""
    d = descriptors[strict]
    print(f"k_render_bwd_tile_step<{strict}>: next_free_vgpr {d['next_free_vgpr']}, private segment "
          f"{d['private_segment_fixed_size']} B, LDS {d['group_segment_fixed_size']} B")
    assert d["next_free_vgpr"] <= 64
    assert d["private_segment_fixed_size"] == 0
    assert d["group_segment_fixed_size"] <= 5120
