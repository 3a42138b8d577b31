"""The wait states of the hand-written asm loops (vrt_march.h's march step, vrt_path.hip's VBM_* bounce march), on the CPU.

hipcc pads the hazards of the code it generates and nothing inside an `asm` string.  tools/isa_hazards.py scans the device assembly
of every translation unit with kernels (the Makefile's flags + --cuda-device-only -S: `make asm`) for a producer -> consumer pair with
fewer wait states between them than gfx950 needs.  Each rule it applies is held to the toolchain here by a probe: a few lines of HIP
whose hipcc output pads the pair (the rule is no stricter than hipcc), and the same pair unpadded in an asm string (the checker finds
it).  Zero findings in compiler-generated code calibrates the checker; zero inside inline asm is the property the loops must keep.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazards as hz  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

if not os.path.exists(HIPCC):
    pytest.skip("hipcc is not installed", allow_module_level=True)

RULES = {r.name: r for r in hz.RULES}

# rule -> (kernel hipcc pads, the same pair in an asm string, producer mnemonic, consumer mnemonic)
PROBES = {
    "valu_sgpr_valu": (
        """extern "C" __global__ void hp_valu_sgpr_valu(const float *a, const float *b, float *o) {
             int i = threadIdx.x; o[i] = a[i] == b[i] ? a[i + 64] : b[i + 64]; }""",
        """extern "C" __global__ void ap_valu_sgpr_valu(const float *a, float *o) {
             int i = threadIdx.x; float r;
             asm volatile("v_cmp_eq_f32_e32 vcc, %1, %2\\n\\tv_cndmask_b32_e32 %0, %1, %2, vcc" : "=v"(r) : "v"(a[i]), "v"(a[i + 64]) : "vcc");
             o[i] = r; }""",
        r"v_cmp_eq_f32", r"v_cndmask_b32"),
    "valu_sgpr_lanesel": (
        """extern "C" __global__ void hp_valu_sgpr_lanesel(const int *a, int *o) {
             int i = threadIdx.x; int v = a[i];
             o[i] = __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(v) & 63); }""",
        """extern "C" __global__ void ap_valu_sgpr_lanesel(const int *a, int *o) {
             int i = threadIdx.x; int t, r;
             asm volatile("v_readfirstlane_b32 %0, %2\\n\\tv_readlane_b32 %1, %2, %0" : "=&s"(t), "=s"(r) : "v"(a[i]));
             o[i] = r; }""",
        r"v_readfirstlane_b32", r"v_readlane_b32"),
    "valu_sgpr_vmem": (
        """extern "C" __global__ void hp_valu_sgpr_vmem(const int *a, int *o) {
             int i = threadIdx.x; int s = __builtin_amdgcn_readfirstlane(a[i]);
             __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)a, 0, 0x10000, 0x00020000);
             o[i] = __builtin_amdgcn_raw_buffer_load_b32(r, i * 4, s, 0); }""",
        """extern "C" __global__ void ap_valu_sgpr_vmem(const int *a, int *o) {
             int i = threadIdx.x; int r, s;
             __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc((void *)a, 0, 0x10000, 0x00020000);
             asm volatile("v_readfirstlane_b32 %1, %2\\n\\tbuffer_load_dword %0, %3, %4, %1 offen\\n\\ts_waitcnt vmcnt(0)"
                          : "=v"(r), "=&s"(s) : "v"(a[i]), "v"(i * 4), "s"(d) : "memory");
             o[i] = r; }""",
        r"v_readfirstlane_b32", r"buffer_load_dword"),
    "valu_vgpr_readlane": (
        """extern "C" __global__ void hp_valu_vgpr_readlane(const int *a, int *o) {
             int i = threadIdx.x; o[i] = __builtin_amdgcn_readfirstlane(a[i] + a[i + 64]); }""",
        """extern "C" __global__ void ap_valu_vgpr_readlane(const int *a, int *o) {
             int i = threadIdx.x; int r, t;
             asm volatile("v_add_u32_e32 %1, %2, %2\\n\\tv_readfirstlane_b32 %0, %1" : "=s"(r), "=&v"(t) : "v"(a[i]));
             o[i] = r; }""",
        r"v_add_u32", r"v_readfirstlane_b32"),
    "trans_valu": (
        """extern "C" __global__ void hp_trans_valu(const float *a, float *o) {
             int i = threadIdx.x; float x = a[i]; o[i] = __builtin_amdgcn_exp2f(x) * x; }""",
        """extern "C" __global__ void ap_trans_valu(const float *a, float *o) {
             int i = threadIdx.x; float r, t;
             asm volatile("v_exp_f32_e32 %1, %2\\n\\tv_mul_f32_e32 %0, %1, %2" : "=v"(r), "=&v"(t) : "v"(a[i]));
             o[i] = r; }""",
        r"v_exp_f32", r"v_mul_f32"),
}


def test_every_rule_has_a_probe():
    assert set(PROBES) == set(RULES)


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    """Every probe kernel, compiled with the product's flags; {kernel name: Function}."""
    d = tmp_path_factory.mktemp("probes")
    src = d / "probes.hip"
    src.write_text("#include <hip/hip_runtime.h>\n" + "\n".join(p[0] + "\n" + p[1] for p in PROBES.values()) + "\n")
    out = d / "probes.s"
    subprocess.check_call([HIPCC, *hz.hipflags(), "--cuda-device-only", "-S", "-o", str(out), str(src)], stderr=subprocess.DEVNULL)
    return {f.name: f for f in hz.parse(out.read_text())}


def _pairs(fn, rule, prod, cons, horizon):
    return [f for f in hz.scan([fn], rules=[rule], horizon=horizon)
            if re.match(prod, f.producer.op) and re.match(cons, f.consumer.op)]


@pytest.mark.parametrize("name", sorted(PROBES))
def test_hipcc_pads_each_rule_at_least_as_much(probes, name):
    """What hipcc emits for the pair in its own code: at least the rule's wait states (the rule is no stricter than the toolchain)."""
    rule, (_, _, prod, cons) = RULES[name], PROBES[name]
    found = _pairs(probes[f"hp_{name}"], rule, prod, cons, horizon=rule.need + 8)
    assert found, f"hipcc's code for the {name} probe has no {prod} -> {cons} pair: the probe no longer shows the rule"
    assert all(not f.in_asm for f in found)
    assert min(f.found for f in found) >= rule.need, "\n".join(map(str, found))


@pytest.mark.parametrize("name", sorted(PROBES))
def test_checker_flags_each_rule_unpadded_in_asm(probes, name):
    rule, (_, _, prod, cons) = RULES[name], PROBES[name]
    bad = [f for f in _pairs(probes[f"ap_{name}"], rule, prod, cons, horizon=None) if f.violation]
    assert bad and all(f.in_asm for f in bad) and min(f.found for f in bad) == 0


# ---- the walk itself, on hand-written text ----
def _fn(body):
    text = "k:\n" + "\n".join(";;#ASMSTART" if l == "{" else ";;#ASMEND" if l == "}" else "\t" + l for l in body) + "\n\ts_endpgm\n"
    return hz.parse(text)


def test_walk_counts_nops_and_stops_at_the_rule():
    rule = RULES["valu_sgpr_valu"]
    assert [f.found for f in hz.violations(_fn(["{", "v_cmp_eq_f32_e32 vcc, v1, v2", "v_cndmask_b32_e32 v3, v1, v2, vcc", "}"]))] == [0]
    assert [f.found for f in hz.violations(_fn(["{", "v_cmp_eq_f32_e32 vcc, v1, v2", "s_nop 0", "v_cndmask_b32_e32 v3, v1, v2, vcc", "}"]))] == [1]
    assert not hz.violations(_fn(["{", "v_cmp_eq_f32_e32 vcc, v1, v2", "s_nop 1", "v_cndmask_b32_e32 v3, v1, v2, vcc", "}"]))
    assert not hz.violations(_fn(["v_cmp_eq_f32_e64 s[4:5], v1, v2", "v_mov_b32_e32 v0, 0", "v_mov_b32_e32 v9, 0",
                                  "v_cndmask_b32_e64 v3, v1, v2, s[4:5]"]))
    # an SGPR pair, half of it read; a redefinition by the scalar unit ends the hazard
    assert [f.found for f in hz.violations(_fn(["v_cmp_eq_f32_e64 s[4:5], v1, v2", "v_add_u32_e32 v3, s5, v1"]))] == [0]
    assert not hz.violations(_fn(["v_cmp_eq_f32_e64 s[4:5], v1, v2", "s_mov_b64 s[4:5], 0", "v_cndmask_b32_e64 v3, v1, v2, s[4:5]"]))
    assert rule.need == 2


def test_walk_follows_branches_and_back_edges():
    # the consumer at the loop's head, the producer at its foot: reached through the back-edge (one state: the branch)
    loop = ["{", ".Lhead:", "v_cndmask_b32_e32 v3, v1, v2, vcc", "v_add_f32_e32 v1, v1, v2",
            "v_cmp_eq_f32_e32 vcc, v1, v2", "s_cbranch_scc0 .Lhead", "}"]
    assert [(f.producer.op, f.found) for f in hz.violations(_fn(loop))] == [("v_cmp_eq_f32_e32", 1)]
    # a taken branch past the padding of the fall-through
    jump = ["{", "v_cmp_eq_f32_e32 vcc, v1, v2", "s_cbranch_scc1 .Lt", "s_nop 4", ".Lt:", "v_cndmask_b32_e32 v3, v1, v2, vcc", "}"]
    assert [f.found for f in hz.violations(_fn(jump))] == [1]
    # an unconditional branch does not fall through
    away = ["{", "v_cmp_eq_f32_e32 vcc, v1, v2", "s_branch .Lt", "v_cndmask_b32_e32 v3, v1, v2, vcc", ".Lt:", "s_nop 1",
            "v_cndmask_b32_e32 v4, v1, v2, vcc", "}"]
    assert not hz.violations(_fn(away))
    # compiler code against asm
    assert not hz.violations(_fn(["v_cmp_eq_f32_e32 vcc, v1, v2", "v_cndmask_b32_e32 v3, v1, v2, vcc"]))[0].in_asm


# ---- the product ----
@pytest.fixture(scope="module")
def product(tmp_path_factory):
    """{unit: [Function]} for every translation unit with kernels, built by `make asm` with the Makefile's flags."""
    files = hz.build_asm(str(tmp_path_factory.mktemp("asm")))
    out = {}
    for unit, path in files.items():
        with open(path) as f:
            out[unit] = hz.parse(f.read())
    return out


def test_the_scan_sees_the_asm_loops(product):
    """The march step and the bounce march are in the scanned text, inside asm markers, with their axis selects found as pairs."""
    for unit in ("vrt_kernels", "vrt_path"):
        sel = [f for f in hz.scan(product[unit], rules=[RULES["valu_sgpr_valu"]], horizon=8)
               if f.in_asm and f.producer.op.startswith("v_cmp_eq_f32") and f.consumer.op.startswith("v_cndmask_b32")]
        assert len(sel) >= 3, unit
    labels = {l for fn in product["vrt_path"] for l in fn.labels}
    assert any(l.startswith(".Lvbm_move_") for l in labels) and any(l.startswith(".Lvrt_move_") for l in labels)


@pytest.mark.parametrize("unit", hz.PRODUCT_UNITS)
def test_compiler_generated_code_has_no_violation(product, unit):
    """Calibration: hipcc pads its own code, so a finding here is the checker's error, not the kernel's."""
    bad = [v for v in hz.violations(product[unit]) if not v.in_asm]
    assert not bad, "\n".join(map(str, bad[:20]))


@pytest.mark.parametrize("unit", hz.PRODUCT_UNITS)
def test_inline_asm_has_no_violation(product, unit):
    bad = [v for v in hz.violations(product[unit]) if v.in_asm]
    assert not bad, f"{len(bad)} pair(s) inside inline asm with too few wait states:\n" + "\n".join(map(str, bad[:40]))


@pytest.mark.parametrize("unit", hz.PRODUCT_UNITS)
def test_inline_asm_holds_nothing_no_rule_covers(product, unit):
    """A VALU write of EXEC or a write of M0 inside an asm string would need a rule (and a probe) this checker does not have."""
    assert not hz.uncovered(product[unit])
