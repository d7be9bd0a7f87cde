"""Register budget of the SpGEMM's numeric kernel, read from the gfx950 code object inside the built library (no GPU needed).

The reads-path instantiation of k_spgemm_direct (template flag SPEC, OvSpecParams) exists to drop the scalars the general kernel holds for
switches that a reads-built matrix always sets the same way: the general kernel spills ~120 SGPRs to VGPR lanes.  The SPEC kernels must not spill
VGPRs or use scratch, must stay at or below 80 VGPRs (six waves per SIMD: LDS, not registers, limits the 512-lane tier to three workgroups per CU)
and must spill at most half the SGPRs of the general kernel of the same block size."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "elba_amd", "lib", "libelba_amd.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BLOCKS = (128, 256, 512, 1024)


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def _kernel_notes():
    """{mangled kernel name: {field: int}} from the AMDGPU metadata notes of every gfx950 code object in the library"""
    tools = [_tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or None in tools:
        pytest.skip("library not built, or the LLVM tools are missing")
    objcopy, bundler, readelf = tools
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, os.path.join(tmp, "stripped")])
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)] + [len(data)]      # one bundle per translation unit
        for n in range(len(starts) - 1):
            bundle, co = os.path.join(tmp, "b%d" % n), os.path.join(tmp, "b%d.co" % n)
            open(bundle, "wb").write(data[starts[n]:starts[n + 1]])
            subprocess.check_call([bundler, "--unbundle", "--type=o", "--input=" + bundle, "--targets=" + TARGET, "--output=" + co])
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            cur = None
            for line in notes.splitlines():
                m = re.match(r"\s*-?\s*\.name:\s+(\S+)", line)
                if m:
                    cur = out.setdefault(m.group(1), {})
                    continue
                m = re.match(r"\s*\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", line)
                if m and cur is not None:
                    cur[m.group(1)] = int(m.group(2))
    return out


def _direct(notes, block, spec):
    # k_spgemm_direct<BLOCK, GLOBAL = false, PAY = false, DK = 0, SUFFIX = false, TB = 0, SPEC>
    key = "k_spgemm_directILi%dELb0ELb0ELi0ELb0ELi0ELb%dE" % (block, 1 if spec else 0)
    hits = [v for k, v in notes.items() if key in k]
    assert len(hits) == 1, (key, len(hits))
    return hits[0]


def test_reads_path_numeric_kernels_spill_no_vgprs_and_few_sgprs():
    notes = _kernel_notes()
    for b in BLOCKS:
        spec, gen = _direct(notes, b, True), _direct(notes, b, False)
        assert spec["vgpr_spill_count"] == 0, (b, spec)
        assert spec["private_segment_fixed_size"] == 0, (b, spec)
        assert spec["vgpr_count"] <= 80, (b, spec)
        assert 2 * spec["sgpr_spill_count"] <= gen["sgpr_spill_count"], (b, spec, gen)
