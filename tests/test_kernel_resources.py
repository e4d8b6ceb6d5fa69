"""What the compiler allotted to every kernel of libplp_front.so (csrc/build/*.remarks, written by the Makefile with
-Rpass-analysis=kernel-resource-usage): no kernel of the library may use scratch memory (the generic matcher kernels kept
a 36 / 68-byte frame and spilled 81-125 scalar registers until they were instantiated per family of modes), and the register / LDS
footprints that DESIGN.md section 6 argues with (how many waves of a kernel fit beside two region growers per SIMD) are what the build has."""
import glob
import os
import re

import pytest

BUILD = os.path.join(os.path.dirname(__file__), "..", "structure-plp-slam_amd", "csrc", "build")


def kernels():
    out = {}
    for path in glob.glob(os.path.join(BUILD, "*.remarks")):
        name = None
        for line in open(path, errors="replace"):
            m = re.search(r"remark: (?:[^:]+:\d+:\d+: )?\s*Function Name: (\S+)", line) or re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {"file": os.path.basename(path)}
                continue
            m = re.search(r"remark:(?: [^:\s]+:\d+:\d+:)?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
            if m and name:
                out[name][m.group(1).strip()] = int(m.group(2))
    return out


K = kernels()
needs_build = pytest.mark.skipif(not K, reason="csrc/build/*.remarks absent: run __graft_entry__.build() (make) first")


def find(sub):
    hits = [v for k, v in K.items() if sub in k]
    assert hits, sub
    return hits


@needs_build
def test_every_kernel_was_seen_and_none_uses_scratch():
    assert len(K) >= 45, sorted(K)
    bad = {k: v["ScratchSize"] for k, v in K.items() if v.get("ScratchSize", 0) != 0}
    assert not bad, bad
    assert not {k: v["VGPRs Spill"] for k, v in K.items() if v.get("VGPRs Spill", 0)}, "vector registers spilled"


@needs_build
def test_footprints_the_design_argues_with():
    # beside two growers per SIMD (2 x 147 -> 2 x 152 allotted of 512 VGPRs): 208 registers left
    (grow,) = find("k_lsd_growENS")
    assert grow["VGPRs"] <= 120, grow             # 151 until round 5: the wave's frame index is declared wave-uniform, so every per-frame pointer is scalar (113)
    # the exact seed sort: the builds of it that page-faulted beside other kernels (profiles/r05_seed_sort.md; cause not identified) all carried the scan pass's per-thread
    # register arrays and 150+ spilled SGPRs; staged through LDS the kernel holds 85 registers -- a footprint of the old kind must not come back unnoticed
    for k in find("k_lsd_seed_sort"):
        assert k["VGPRs"] <= 128, k
    (mw,) = find("k_lsd_grow_mw")
    assert mw["VGPRs"] <= 176, mw                 # eight waves of a workgroup on four SIMDs: 2 x 176 <= 512
    # kernels that run at few waves per SIMD even alone: their footprint is their speed.  Beside two growers per SIMD a kernel of
    # at most 64 VGPRs gets three waves, of at most 104 two
    (cells,) = find("k_match_topk_cells")
    assert cells["VGPRs"] <= 64, cells            # 97 at the start of round 3 (one wave beside the growers), 72 (two), now three
    (prep,) = find("k_match_prep")
    assert prep["LDS Size"] <= 34 * 1024, prep    # two workgroups in the 77 KB the growers leave on a CU (was 41 KB: one)
    (srt,) = find("k_match_resolve_sorted")
    assert srt["VGPRs"] <= 128, srt
    (qt,) = find("k_quadtree")
    assert qt["VGPRs"] <= 64, qt                  # 68 with the sixteen per-value ballots of the radix ranking
    (lbd,) = find("k_lbdENS")
    assert lbd["VGPRs"] <= 64, lbd                # 76 with the f64 cos / sin of the line direction computed by all 64 lanes of the line's wave
    (sob,) = find("k_blur_sobel")
    assert sob["LDS Size"] <= 15 * 1024, sob      # five workgroups beside the growers (18.5 KB: four)
    for name in ("k_fast_cells", "k_blur7", "k_resize_linear"):
        for k in find(name):
            assert k["VGPRs"] <= 72, (name, k)
    (rb,) = find("k_orient_rbrief")
    assert rb["VGPRs"] <= 80 and rb["LDS Size"] <= 31 * 1024, rb   # five workgroups per CU alone (LDS), two beside the growers
    # the per-family instantiations of the generic matcher kernels exist (line, group, point)
    for name in ("k_match_topk_lanesILi", "k_match_topkILi", "k_match_resolve_genericILi"):
        assert len(find(name)) == 3, name


# Scalar registers spilled into VGPR lanes (a v_writelane / v_readlane pair each time one is used), per kernel.  VERDICT r05: the chain-bound kernels -- one instruction
# per ~15 cycles -- pay for every one of them on their critical path, and every build of the seed sort that ever faulted beside other kernels carried 150+ of them
# (profiles/r05_seed_sort.md), so the number is RECORDED per kernel and held: a kernel not listed may spill at most kSpillDefault, a listed one at most its figure.
# Lower a cap when a kernel's spills go down; raising one needs a reason in the line's comment.
kSpillDefault = 20
SPILL_CAPS = {
    "k_lsd_growENS": 72,                 # round 5: 72 (the loop state of region_grow + rectangle fit + refinement live across the round loop)
    "k_lsd_grow_mw": 175,                # round 5: 175 -- the latency path's kernel; soaked beside other kernels by tests/test_gpu_concurrent_single_frame.py
    "k_match_resolve_sorted": 69,
    "k_match_resolve_genericILi1": 51,
    "k_match_resolve_genericILi2": 44,
    "k_match_resolve_genericILi3": 64,
    "k_quadtree": 48,                    # 39 in round 5, 44 now: the radix counters and sorted keys are reached through dual-address-space accessors (DS / GLOBAL behind a scalar branch: no FLAT access); two inlined copies of the code had cost 83
    "k_lsd_seed_sort": 32,               # round 6: 29 (8 in round 5): wave_sub_sort / wave_reg_sort keep their stacks, chunk masks and prefix sums in scalar registers by design
    "k_seed_sort_debug": 48,             # the test entry of the same body, with the phase clocks
}


def spill_table():
    return {k: v.get("SGPRs Spill", 0) for k, v in K.items()}


@needs_build
def test_spilled_scalar_registers_are_recorded_and_capped():
    over = {}
    for name, n in spill_table().items():
        cap = next((c for sub, c in SPILL_CAPS.items() if sub in name), kSpillDefault)
        if n > cap:
            over[name] = (n, cap)
    assert not over, f"spilled SGPRs above the recorded cap (kernel: (now, cap)): {over}"
    for sub in SPILL_CAPS:               # every listed kernel still exists under that name
        find(sub)


def test_the_build_pins_the_cache_mode_the_workgroup_scope_hand_overs_need():
    """k_lsd_grow_mw's region lists and the seed sort's global partitions go from wave to wave through HBM at workgroup scope: valid only without threadgroup split"""
    mk = open(os.path.join(BUILD, "..", "Makefile")).read()
    flags = next(l for l in mk.splitlines() if l.startswith("FLAGS"))
    assert "-mno-tgsplit" in flags and "-mtgsplit" not in flags.replace("-mno-tgsplit", ""), flags


def isa_files():
    return sorted(glob.glob(os.path.join(BUILD, "*.s")))


@pytest.mark.skipif(not isa_files(), reason="csrc/build/*.s absent: run __graft_entry__.build() (make keeps the device ISA of every translation unit)")
def test_no_kernel_reaches_memory_through_flat_instructions():
    """A pointer whose address space the compiler does not know (`fits ? lds : hbm`, a pointer made from an integer) is reached through FLAT loads and stores: an aperture check
    per access, both wait counters held, no scalar-base addressing.  Three kernels had them until round 6 (k_quadtree, k_lsd_grow_mw, k_match_topk_cells); each is now specialised
    per address space (DS instructions for LDS, scalar-base GLOBAL instructions for HBM) and this test keeps the library free of them.  (Round 6 first read the seed sort's failure
    beside a second dispatch as a property of FLAT / vector-address accesses; it was a barrier that had lost its wait -- see the next test.)"""
    bad = {}
    for path in isa_files():
        kernel = None
        for line in open(path, errors="replace"):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                kernel = m.group(1)
            elif re.match(r"^\s+flat_(load|store|atomic)", line):
                bad[kernel] = bad.get(kernel, 0) + 1
    assert not bad, f"FLAT memory instructions (kernel: count): {bad}"


def _barrier_check():
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_barrier_check", os.path.join(os.path.dirname(__file__), "..", "tools", "isa_barrier_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_barrier_check_sees_a_wait_that_is_missing_on_the_back_edge_only(tmp_path):
    """the shape the compiler produced (profiles/r06_seed_sort.md section 4): nothing pending on the way in, an LDS write pending on the loop's back edge, no wait at the header"""
    chk = _barrier_check()
    text = """_Zkernel:
\ts_load_dword s0, s[4:5], 0x0
\ts_branch .LBB0_2
.LBB0_1:
\tds_write_b32 v2, v3 offset:64
.LBB0_2:
{wait}\ts_barrier
\tds_read_b32 v3, v2 offset:64
\ts_waitcnt lgkmcnt(0)
\tv_readfirstlane_b32 s2, v3
\ts_cmp_eq_u32 s2, 0
\ts_cbranch_scc0 .LBB0_1
\ts_endpgm
.Lfunc_end0:
"""
    for wait, want in (("", 1), ("\ts_waitcnt lgkmcnt(0)\n", 0), ("\ts_waitcnt vmcnt(0)\n", 1), ("\ts_waitcnt vmcnt(0) lgkmcnt(0)\n", 0)):
        f = tmp_path / "k.s"
        f.write_text(text.format(wait=wait))
        (name, body), = list(chk.kernels(str(f)))
        assert name == "_Zkernel" and len(chk.check(body)) == want, (wait, chk.check(body))


@pytest.mark.skipif(not isa_files(), reason="csrc/build/*.s absent: run __graft_entry__.build() (make keeps the device ISA of every translation unit)")
def test_every_barrier_is_reached_with_the_waves_lds_writes_drained():
    """THE CAUSE of the failure of rounds 4 - 6 (profiles/r06_seed_sort.md section 4): the `s_waitcnt lgkmcnt(0)` of __syncthreads()'s release fence is a soft wait, and the
    compiler deleted it at the barrier that heads the seed sort's loop over global partitions in some builds (nothing pending on the path from the entry; wave 0's pushes to
    the segment stack pending on the back edge).  The other waves then read the stack early -- beside a second dispatch, whose LDS traffic stretches the window, every time.
    The library's barriers carry a hard wait (csrc/plp_barrier.hpp); this test proves on the kept ISA, by data-flow over the basic blocks of every kernel, that no s_barrier can
    be reached while an LDS write of the arriving wave may still be in flight."""
    chk = _barrier_check()
    bad, seen = {}, 0
    for path in isa_files():
        for name, body in chk.kernels(path):
            if any(re.match(r"^\s+s_barrier", l) for _, l in body):
                seen += 1
                lines = chk.check(body)
                if lines:
                    bad[name] = lines
    assert seen >= 20, seen
    assert not bad, f"barriers reached with LDS writes in flight (kernel: lines of csrc/build/*.s): {bad}"
    # ... and the sources do not go back to the soft form
    src = os.path.join(BUILD, "..")
    for path in glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.inc")) + glob.glob(os.path.join(src, "*.hpp")):
        if os.path.basename(path) == "plp_barrier.hpp":
            continue
        for no, line in enumerate(open(path), 1):
            code = line.split("//")[0]
            assert "__syncthreads()" not in code, f"{os.path.basename(path)}:{no}: use wg_barrier() (csrc/plp_barrier.hpp)"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_25_line_reproducer_of_the_deleted_wait_and_its_cure(tmp_path):
    """tools/experiments/soft_wait_loop_header.hip: with __syncthreads() this compiler leaves the loop header's s_barrier without its LDS wait (on the hardware: half of all thread
    results wrong, git show 09a8f08:tools/sessions/r06/run56.sh); with the hard wait of csrc/plp_barrier.hpp the barrier is reached clean (0 wrong).  The cure is asserted; the defect is reported
    (a compiler that no longer shows it makes this test say so, not fail)."""
    import subprocess
    chk = _barrier_check()
    src = os.path.join(os.path.dirname(__file__), "..", "tools", "experiments", "soft_wait_loop_header.hip")
    found = {}
    for name, flag in (("soft", []), ("hard", ["-DHARD_WAIT"])):
        out = tmp_path / f"{name}.s"
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-mno-tgsplit", "-DWITH_MAIN", "--cuda-device-only", "-S", "-o", str(out), src] + flag,
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        (kname, body), = [kb for kb in chk.kernels(str(out)) if kb[0].startswith("_Z1k")]
        found[name] = chk.check(body)
    assert found["hard"] == [], found
    if not found["soft"]:
        pytest.skip("this compiler keeps the wait of __syncthreads() at the loop header: the defect of ROCm 7.2 is not present")
