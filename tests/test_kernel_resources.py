"""Register / scratch budget of the performance-critical kernels, read from the built objects (no GPU needed).  The
kernels are designed against fixed occupancies -- two waves per SIMD at 256 registers for the fused sampler and the
block-shared tangent kernel -- and a change that pushes spill code into their loops costs far more than it looks
(scratch is vector memory: in the tangent kernel every spill waits behind the LDS-DMA prefetch window)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _kernels(obj, tmp):
    fb, co = os.path.join(tmp, "_kr_test.fb"), os.path.join(tmp, "_kr_test.co")
    # (an explicit output file: objcopy without one rewrites its input, and a touched object makes the next build() rebuild)
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "_kr_test.o")],
                   check=True, capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                         r"\.vgpr_count:\s+(\d+)", txt, re.S):
        ag, name, scr, vg = m.groups()
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(.*", "", dem).replace("void pita::", "")] = dict(vgpr=int(vg), agpr=int(ag), scratch=int(scr))
    return out


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-readelf") or shutil.which("c++filt") is None,
                    reason="needs the ROCm LLVM binutils")
def test_register_and_scratch_budgets(tmp_path):
    import pita_amd.build as build

    build.build(verbose=False)
    k = {}
    for f in ("egnn_kernel.o", "egnn_div_kernel.o", "energy_kernels.o"):
        k.update(_kernels(os.path.join(ROOT, "pita_amd", "csrc", f), str(tmp_path)))
    # fused sampler, default precision, every instantiated system: two waves per SIMD (<= 256 registers in total), its
    # spill code stays outside the edge loop (140 B/lane for LJ13 today)
    for name in ("egnn_kernel<13, 3, 7, 4, 2, true, 2>", "egnn_kernel<4, 2, 8, 4, 2, true, 2>",
                 "egnn_kernel<22, 3, 4, 4, 2, true, 2>", "egnn_kernel<55, 3, 1, 4, 2, true, 2>"):
        r = k[name]
        assert r["vgpr"] + r["agpr"] <= 256 and r["scratch"] <= 256, (name, r)
    # block-shared tangent kernels: 256 registers and (almost) no spill -- scratch is vector memory, and inside the LDS-DMA
    # stream a spill waits behind the whole prefetch window (round 4: the layer sweep in three instantiations; what is
    # left, 48 B/lane for LJ13, sits in the per-group set-up, outside the stream's item loops)
    for name, lim in (("egnn_div_tangent_shared_kernel<13, 3, 2, 8, 2>", 64), ("egnn_div_tangent_shared_kernel<22, 3, 1, 8, 2>", 64),
                      ("egnn_div_tangent_shared_kernel<55, 3, 1, 8, 1>", 0)):
        r = k[name]
        assert r["vgpr"] + r["agpr"] <= 256 and r["scratch"] <= lim, (name, r)
    # the cache writer (round 4: no direction of its own) must not spill at all (one wave per SIMD, 512 registers)
    assert k["egnn_div_fast_kernel<13, 3, 2, 4, 0, 0, 1>"]["scratch"] == 0
    # target kernels: no scratch (the fused MALA chain carries two force sets and spills a little between its phases)
    for name, r in k.items():
        if name.startswith("lj13_mala"):
            assert r["scratch"] <= 192, (name, r)
        elif name.startswith("lj13_") or name.startswith("pair_"):
            assert r["scratch"] == 0, (name, r)


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="needs the ROCm LLVM binutils")
def test_packed_fp32_exposure_of_shipped_kernels():
    """Object-level record of how exposed the SHIPPED kernels are to the instruction form behind round 5's run-to-run
    differences (v_pk_{mul,add,fma}_f32 with an SGPR-pair source and op_sel, profiles/r05_walker_packed_fp32_hazard.txt):
    profiles/r06_packed_fp32_exposure.txt (tools/packed_fp32_audit.py) lists the counts per kernel; this test recomputes
    the per-object totals from the objects on disk and requires the committed listing to be current, the headline objects
    to be in it, and the one matrix instruction the fault was seen beside (16x16x32) to be absent from the library.  The
    run-time side is tests/test_hip_parity.py::test_default_path_full_batch_rerun."""
    import sys

    import pita_amd.build as build

    build.build(verbose=False)
    assert build.fallback_objects() == [], build.fallback_objects()  # the record of the build that made the library on disk
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import packed_fp32_audit as A

    committed = {}
    for ln in open(os.path.join(ROOT, "profiles", "r06_packed_fp32_exposure.txt")):
        f = ln.split()
        if len(f) >= 9 and f[-2:] == ["(whole", "object)"]:
            committed[f[0]] = tuple(int(v) for v in f[1:5])
    now = {}
    for obj in A.shipped_objects():
        k = A.audit_object(obj)
        now[os.path.basename(obj)] = tuple(sum(r[f] for r in k.values()) for f in ("pk", "sgpr", "opsel", "both"))
        assert all(r["mfma16"] == 0 for r in k.values()), obj  # no v_mfma_f32_16x16x32_* ships
    assert now == committed, ("profiles/r06_packed_fp32_exposure.txt is stale: python tools/packed_fp32_audit.py > "
                              "profiles/r06_packed_fp32_exposure.txt", now, committed)
    for obj in ("egnn_kernel.o", "egnn_div_kernel.o", "egnn_vjp_kernel.o", "mlp_kernel.o"):
        assert committed[obj][3] > 0  # the exposure is real and on record (round-5 review: 1 202 / 1 982 / 2 155 / 2 192)


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="needs the ROCm LLVM binutils")
def test_issue_priorities_are_in_the_built_kernels(tmp_path):
    """Round 5: the fused sampler's three SiLUs per edge and the block-shared tangent kernel's operand split run at the lower
    issue priority (s_setprio; DESIGN 4.1 viii: -6 % / -4.5 %, bit-identical results).  The scalar instructions must be in
    the objects that ship: six per unrolled edge and column tile in the sampler, two per edge item in the tangent kernel."""
    import pita_amd.build as build

    build.build(verbose=False)
    for obj, needle, least in (("egnn_kernel.o", "egnn_kernelILi13ELi3ELi7ELi4ELi2ELb1ELi2E", 18),
                               ("egnn_div_kernel.o", "egnn_div_tangent_shared_kernelILi13ELi3ELi2ELi8ELi2E", 2)):
        _kernels(os.path.join(ROOT, "pita_amd", "csrc", obj), str(tmp_path))  # leaves the device code object in tmp_path
        asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", str(tmp_path / "_kr_test.co")], check=True, capture_output=True,
                             text=True).stdout
        start = asm.index(f"<_ZN4pita{len(needle.split('IL')[0])}{needle}")
        body = asm[start:asm.index("s_endpgm", start)]
        assert body.count("s_setprio") >= least, (obj, body.count("s_setprio"))
