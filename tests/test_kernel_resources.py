"""Register / scratch / LDS budget of the hot kernels, from hipcc's own resource report (-Rpass-analysis=kernel-resource-usage),
in the build container: a toolchain change (or an edit) that spills, drops occupancy or outgrows the CU's LDS fails HERE, next
to tests/test_disasm_guard.py, instead of showing up as a slower or failing launch on the GPU box.

The budgets are what the design rests on: the 16-wave run kernels hold one workgroup per CU — 4 waves per SIMD,
so at most 128 VGPRs, no scratch (a scratch reload waits for the PCM stores in flight), at most 160 KiB of LDS; the eight-wave
ones hold two workgroups per CU, so the same registers and at most 80 KiB of LDS each.

Every registered run kernel is checked: the rows of aac.js_amd/csrc/aacg_run_kernels.h, in the translation unit that expands
their list (AACG_RUN_KERNEL_UNIT), built with the flags the Makefile builds that unit with."""
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aac.js_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
BUDGET = {"AACG_WG_WAVES": (128, 4, 160 * 1024), "AACG_HALF_WAVES": (128, 4, 80 * 1024)}   # (max VGPRs, min waves/SIMD, max LDS bytes)


def registry():
    """{list macro: [(kernel, wave count macro)]} from the rows of aacg_run_kernels.h"""
    with open(os.path.join(CSRC, "aacg_run_kernels.h")) as f:
        text = f.read().replace("\\\n", " ")
    lists = {}
    for m in re.finditer(r"^#define (AACG_RUN_KERNELS_\w+)\(X\)(.*)$", text, re.M):
        rows = re.findall(r"X\(\s*(\w+)\s*,[^,()]*,\s*(\w+)\s*,\s*\w+\s*\)", m.group(2))
        lists[m.group(1)] = [("aacg_imdct_run_" + suffix, waves) for suffix, waves in rows]
    return lists


def units():
    """{translation unit: [(kernel, wave count macro)]}: the file that expands each list"""
    lists, out = registry(), {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            for name in re.findall(r"^AACG_RUN_KERNEL_UNIT\(\w+, (AACG_RUN_KERNELS_\w+)\)", f.read(), re.M):
                out.setdefault(os.path.basename(path), []).extend(lists.pop(name))
    assert not lists, "registered but expanded nowhere: %s" % sorted(lists)
    return out


TUS = units()


def make_var(name):
    r = subprocess.run(["make", "-s", "-C", CSRC, "print-" + name], capture_output=True, text=True, timeout=60, check=True)
    return shlex.split(r.stdout)


def report_text(tu):
    flags = make_var("CXXFLAGS") + make_var("FLAGS_" + tu[:-len(".hip")])
    r = subprocess.run([HIPCC, "--offload-arch=gfx950"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", tu, "-o", "/dev/null"],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def resource_report(tu):
    out, name = {}, None
    for line in report_text(tu).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


@pytest.fixture(scope="module")
def reports():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        futs = {tu: ex.submit(resource_report, tu) for tu in TUS}
        return {tu: f.result() for tu, f in futs.items()}


def test_rows_read_here_are_the_registered_kernels(engine_lib):
    import aacgpu
    kernels = [k for rows in TUS.values() for k, _ in rows]
    assert sorted(kernels) == sorted(aacgpu.run_kernels()), kernels
    assert all(w in BUDGET for rows in TUS.values() for _, w in rows), TUS


def sgpr_spill_allowance(kernel):
    # scalar spills go to VGPR lanes (no memory traffic); the plain kernels have none, the optional-stage builds a handful
    return 48 if kernel.endswith("_ex_rv") else 32 if kernel.endswith("_ex") else 0


@pytest.mark.parametrize("tu", sorted(TUS))
def test_hot_kernels_keep_their_register_and_lds_budget(reports, tu):
    for kernel, waves in TUS[tu]:
        max_vgpr, min_occ, max_lds = BUDGET[waves]
        rep = reports[tu].get(kernel)
        assert rep, "%s: kernel %s not in the resource report (%s)" % (tu, kernel, sorted(reports[tu]))
        assert int(rep["VGPRs"]) + int(rep["AGPRs"]) <= max_vgpr, (kernel, rep)
        assert int(rep["ScratchSize [bytes/lane]"]) == 0 and int(rep["VGPRs Spill"]) == 0, (kernel, rep)
        assert int(rep["SGPRs Spill"]) <= sgpr_spill_allowance(kernel), (kernel, rep)
        assert int(rep["Occupancy [waves/SIMD]"]) >= min_occ, (kernel, rep)
        assert int(rep["LDS Size [bytes/block]"]) <= max_lds, (kernel, rep)
        assert rep["Dynamic Stack"] == "False", (kernel, rep)


def test_the_makefile_gate_bites():
    """The Makefile's resource gate (GATED, resource_gate.awk), run as its recipe runs it on hipcc's report of the carry unit:
    the report as it is passes; with scratch, without the kernel's entry, or over a VGPR / LDS budget it fails and says why."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    row = [g.split(":") for g in make_var("GATED") if g.startswith("aacg_engine_carry:")]
    assert row == [["aacg_engine_carry", "aacg_units_carry_shape", "-", "-"]], row
    unit, kernel, max_vgprs, max_lds = row[0]
    text = report_text(unit + ".hip")

    def gate(report, vgprs=max_vgprs, lds=max_lds):
        r = subprocess.run(["awk", "-v", "unit=" + unit, "-v", "kernel=" + kernel, "-v", "max_vgprs=%s" % vgprs, "-v", "max_lds=%s" % lds,
                            "-f", os.path.join(CSRC, "resource_gate.awk")], input=report, capture_output=True, text=True, timeout=60)
        return r.returncode, r.stdout

    rc, out = gate(text)
    assert rc == 0 and out.startswith(unit + ": ") and "fails" not in out, (rc, out)
    spoiled, n = re.subn(r"(ScratchSize \[bytes/lane\]: )0 ", r"\g<1>16 ", text)
    assert n == 1
    rc, out = gate(spoiled)
    assert rc != 0 and "scratch=16" in out, (rc, out)
    renamed, n = re.subn(r"(Function Name: )" + kernel + " ", r"\1somebody_else ", text)
    assert n == 1
    rc, out = gate(renamed)
    assert rc != 0 and "no resource report" in out, (rc, out)
    # the headline kernel's two extra budgets, on this report: one below what the kernel uses
    vgprs = int(re.search(r" VGPRs: (\d+) ", text).group(1))
    rc, out = gate(text, vgprs=vgprs - 1)
    assert rc != 0 and "VGPRs=%d" % vgprs in out and "LDS" not in out.splitlines()[-1], (rc, out)
    rc, out = gate(text, vgprs=vgprs)
    assert rc == 0, (rc, out)
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+) ", text).group(1))
    rc, out = gate(text, lds=lds - 1)
    assert rc != 0 and "LDS=%d" % lds in out and "VGPRs=" not in out.splitlines()[-1], (rc, out)
    rc, out = gate(text, lds=lds)
    assert rc == 0, (rc, out)
