"""tools/isa_barrier_check.py against a plain reference (CPU only).

The tool is the build's gate for the compiler defect of DESIGN.md section 5 (a barrier whose LDS wait was deleted), so it is held to a second, deliberately naive
implementation written here: every instruction is its own node with explicit successors, and the two pending states (a DS write, counted on lgkmcnt; an LDS-DMA,
counted on vmcnt) are solved by plain round-robin iteration to a fixpoint.  The two are compared on hand-written cases with known answers, on seeded random functions in
LLVM's textual shape, on every kernel of the build, and on one mutant of the build per s_barrier with the LDS waits in front of it deleted."""
import glob
import importlib.util
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(__file__), "..")
BUILD = os.path.join(ROOT, "structure-plp-slam_amd", "csrc", "build")
HIPCC = "/opt/rocm/bin/hipcc"


def _tool():
    spec = importlib.util.spec_from_file_location("isa_barrier_check", os.path.join(ROOT, "tools", "isa_barrier_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


chk = _tool()


def isa_files():
    return sorted(glob.glob(os.path.join(BUILD, "*.s")))


needs_isa = pytest.mark.skipif(not isa_files(), reason="csrc/build/*.s absent: run __graft_entry__.build() (make keeps the device ISA of every translation unit)")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the reference: one node per instruction, explicit successors, round-robin fixpoint.  Shares nothing with the tool.

READS = ("ds_read", "ds_bpermute", "ds_permute", "ds_swizzle", "ds_nop")


def ref_nodes(lines):
    """[(line_no, mnemonic, operands)] and {label: index of the next instruction} of a function's lines (code in .text sections only)"""
    nodes, labels, text = [], {}, True
    for no, line in lines:
        s = line.split(";")[0].split("//")[0].strip()
        if s.startswith(".section") or s in (".text", ".rodata", ".data", ".bss"):
            text = s == ".text" or s.split()[1].startswith(".text")
            continue
        if not text or not s or s.startswith("."):
            if text and re.fullmatch(r"\.[\w.$]+:", s):
                labels[s[:-1]] = len(nodes)
            continue
        if s.endswith(":"):
            labels[s[:-1]] = len(nodes)
            continue
        parts = s.split(None, 1)
        nodes.append((no, parts[0], parts[1] if len(parts) > 1 else ""))
    return nodes, labels


def ref_check(lines, entry=0):
    """line numbers of the s_barrier nodes whose input state is not empty.  Bit 1: a DS write pending (until lgkmcnt(0)); bit 2: an LDS-DMA pending (until vmcnt(0))."""
    nodes, labels = ref_nodes(lines)
    n = len(nodes)
    succ, gen, kill = [], [], []
    for i, (no, m, ops) in enumerate(nodes):
        if m == "s_branch":
            succ.append([labels[ops.split()[0]]])
        elif m.startswith("s_cbranch_"):
            succ.append([labels[ops.split()[0]], i + 1])
        elif m == "s_endpgm":
            succ.append([])
        elif m == "s_setpc_b64" and entry and ops == "s[30:31]":
            succ.append([])
        elif m == "s_setpc_b64":
            raise ValueError("indirect jump")
        else:
            succ.append([i + 1])
        if any(s >= n for s in succ[-1]):
            raise ValueError("falls off the end")
        g = k = 0
        if m == "s_waitcnt":
            assert "cnt(" in ops, ops
            lg, vm = re.search(r"lgkmcnt\((\d+)\)", ops), re.search(r"vmcnt\((\d+)\)", ops)
            k = (1 if lg and lg.group(1) == "0" else 0) + (2 if vm and vm.group(1) == "0" else 0)
        elif m.split("_")[0] in ("global", "buffer", "scratch", "flat", "tbuffer") and ("_lds" in m or "lds" in ops.replace(",", " ").split()):
            g = 2
        elif m.startswith("ds_") and not m.startswith(READS):
            g = 1
        elif m.startswith(("flat_store", "flat_atomic", "scratch_store", "scratch_atomic")) or m == "s_swappc_b64":
            g = 3
        gen.append(g)
        kill.append(k)
    state = [0] * n
    if n:
        state[0] = entry
    changed = True
    while changed:
        changed = False
        for i in range(n):
            out = (state[i] & ~kill[i]) | gen[i]
            for j in succ[i]:
                if out | state[j] != state[j]:
                    state[j] |= out
                    changed = True
    return sorted(nodes[i][0] for i in range(n) if nodes[i][1] == "s_barrier" and state[i])


def ref_functions(path):
    """{name: [(line_no, text)]} of the functions a file declares with .type ...,@function (own parse, for comparing the tool's discovery)"""
    lines = open(path, errors="replace").read().split("\n")
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", "\n".join(lines), re.M))
    out, cur = {}, None
    for no, line in enumerate(lines, 1):
        head = line.split(":")[0]
        if cur is None and head in names and line.startswith(head + ":"):
            cur = out.setdefault(head, [])
        elif cur is not None and line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append((no, line))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# hand-written cases: the barriers marked `; BAD` are exactly the ones that must be flagged

def flagged(tmp_path, text, name="_Zkernel"):
    f = tmp_path / "k.s"
    f.write_text(text)
    found = {n: b for n, b in chk.kernels(str(f))}
    assert list(found) == [name], list(found)
    body = found[name]
    want = [no for no, line in enumerate(text.split("\n"), 1) if "s_barrier" in line and "; BAD" in line]
    got = chk.check(body)
    assert ref_check(list(body)) == want, (ref_check(list(body)), want)
    return got, want


def test_a_write_before_a_mid_block_branch_reaches_the_taken_edges_barrier(tmp_path):
    """the fall-through block after s_cbranch has no label, so the branch sits in the middle of what a label-only split calls a block"""
    got, want = flagged(tmp_path, """_Zkernel:
\tds_write_b32 v1, v2
\ts_cbranch_scc1 .LBB0_2
; %bb.1:
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\ts_endpgm
.LBB0_2:
\ts_barrier ; BAD
\ts_endpgm
.Lfunc_end0:
""")
    assert got == want == [9]


def test_a_write_after_a_mid_block_branch_does_not_reach_the_taken_edge(tmp_path):
    """the reverse shape: the write follows the branch, so the taken edge is clean (a label-only split reports it, and build() would refuse the tree)"""
    got, want = flagged(tmp_path, """_Zkernel:
\ts_cmp_eq_u32 s0, 0
\ts_cbranch_scc1 .LBB0_2
; %bb.1:
\tds_write_b32 v1, v2
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\tds_write_b32 v1, v3
\ts_endpgm
.LBB0_2:
\ts_barrier
\ts_endpgm
.Lfunc_end0:
""")
    assert got == want == []


@pytest.mark.parametrize("wait, bad", [("", True), ("\ts_waitcnt lgkmcnt(0)\n", True), ("\ts_waitcnt vmcnt(0)\n", True), ("\ts_waitcnt vmcnt(0) lgkmcnt(0)\n", False)])
def test_a_call_leaves_both_states_pending(tmp_path, wait, bad):
    """the callee of s_swappc_b64 may write LDS through DS instructions or DMA: only a wait for both counters after the call makes the barrier clean"""
    got, want = flagged(tmp_path, f"""_Zkernel:
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\ts_swappc_b64 s[30:31], s[16:17]
{wait}\ts_barrier{" ; BAD" if bad else ""}
\ts_endpgm
.Lfunc_end0:
""")
    assert got == want and bool(got) == bad


@pytest.mark.parametrize("load", ["global_load_lds_dwordx4 v[2:3], off", "global_load_lds_dword v1, s[4:5]", "buffer_load_dword v1, s[4:7], 0 offen lds"])
@pytest.mark.parametrize("wait, bad", [("s_waitcnt lgkmcnt(0)", True), ("s_waitcnt vmcnt(1)", True), ("s_waitcnt vmcnt(1) lgkmcnt(0)", True),
                                       ("s_waitcnt vmcnt(0)", False), ("s_waitcnt vmcnt(0) lgkmcnt(0)", False)])
def test_an_lds_dma_is_drained_by_vmcnt_0_only(tmp_path, load, wait, bad):
    """an LDS-DMA is a pending LDS write on the VM counter: lgkmcnt(0) does not drain it, a counted vmcnt(N > 0) does not either"""
    got, want = flagged(tmp_path, f"""_Zkernel:
\tglobal_load_dword v4, v[6:7], off
\t{load}
\t{wait}
\ts_barrier{" ; BAD" if bad else ""}
\ts_endpgm
.Lfunc_end0:
""")
    assert got == want and bool(got) == bad


@pytest.mark.parametrize("op, bad", [("ds_consume v1", True), ("ds_condxchg32_rtn_b64 v[2:3], v1, v[4:5]", True), ("ds_write_addtid_b32 v1", True),
                                     ("ds_cmpswap_b32 v1, v2, v3", True), ("ds_gws_barrier v1", True),
                                     ("ds_read_addtid_b32 v1", False), ("ds_swizzle_b32 v1, v2 offset:swizzle(SWAP,16)", False), ("ds_nop", False)])
def test_every_ds_instruction_writes_unless_it_is_known_to_read(tmp_path, op, bad):
    """the write set fails closed: a DS mnemonic the old allow-list did not name (ds_consume, ds_condxchg32, ds_write_addtid ...) is a write"""
    got, want = flagged(tmp_path, f"""_Zkernel:
\t{op}
\ts_barrier{" ; BAD" if bad else ""}
\ts_endpgm
.Lfunc_end0:
""")
    assert got == want and bool(got) == bad


def test_an_unmangled_kernel_is_found_and_checked(tmp_path):
    """extern "C" kernels have no _Z prefix; functions are found from .type ...,@function, and data symbols around them are not functions"""
    text = """\t.text
\t.type\tk_plain,@function
k_plain:                                ; @k_plain
; %bb.0:
\tds_write_b32 v1, v2
\ts_barrier ; BAD
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel k_plain
\t\t.amdhsa_group_segment_fixed_size 1024
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
\t.type\tc_table,@object
c_table:
\t.long\t1
"""
    got, want = flagged(tmp_path, text, name="k_plain")
    assert got == want == [6]


@pytest.mark.parametrize("code", ["\ts_branch .LBB9_9\n", "\ts_cbranch_scc0 Lnowhere\n", "\ts_cbranch_execz _Zother\n",
                                  "\ts_setpc_b64 s[4:5]\n", "\ts_setpc_b64 s[30:31]\n", "\ts_cbranch_g_fork s[2:3], s[4:5]\n", "\ts_cbranch_join s2\n", "\ts_call_b64 s[30:31], _Zother\n", "\ts_rfe_b64 s[0:1]\n",
                                  "\ts_waitcnt lgkm(0)\n", "\t.long 0xbf8a0000\n"])
def test_control_flow_or_text_the_tool_cannot_follow_is_an_error(tmp_path, code):
    """an unknown branch target, an indirect jump (in a kernel even s[30:31] is no return), fork / join, an unreadable wait and raw code bytes all raise"""
    f = tmp_path / "k.s"
    f.write_text(f"""\t.type\t_Zkernel,@function
_Zkernel:
\tds_write_b32 v1, v2
{code}\ts_waitcnt lgkmcnt(0)
\ts_barrier
\ts_endpgm
.LBB0_1:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Zkernel
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
""")
    (name, body), = list(chk.kernels(str(f)))
    with pytest.raises(ValueError):
        chk.check(body)


def test_falling_off_the_end_and_an_unclosed_function_are_errors(tmp_path):
    f = tmp_path / "k.s"
    f.write_text("_Zkernel:\n\tds_write_b32 v1, v2\n\ts_cbranch_scc0 .LBB0_1\n.LBB0_1:\n\ts_barrier\n.Lfunc_end0:\n")
    (name, body), = list(chk.kernels(str(f)))
    with pytest.raises(ValueError):
        chk.check(body)
    f.write_text("_Zkernel:\n\ts_barrier\n\ts_endpgm\n")
    with pytest.raises(ValueError):
        list(chk.kernels(str(f)))


@pytest.mark.parametrize("wait, bad_ds, bad_dma", [("s_waitcnt 0", False, False), ("s_waitcnt 0xc07f", False, True), ("s_waitcnt 0x0f70", True, False),
                                                   ("s_waitcnt vmcnt(0) & lgkmcnt(0)", False, False), ("s_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)", False, False),
                                                   ("s_waitcnt expcnt(0)", True, True), ("s_waitcnt lgkmcnt(0) vmcnt(63)", False, True)])
def test_every_form_of_s_waitcnt_is_read(wait, bad_ds, bad_dma):
    """named fields in any order and with any separator, and the raw gfx9 immediate (vmcnt bits 3:0 + 15:14, lgkmcnt bits 11:8)"""
    for first, bad in (("ds_write_b32 v1, v2", bad_ds), ("global_load_lds_dword v1, s[4:5]", bad_dma)):
        assert chk.check([(1, "\t" + first), (2, "\t" + wait), (3, "\ts_barrier"), (4, "\ts_endpgm")]) == ([3] if bad else []), (first, wait)


def test_a_device_function_is_entered_with_both_states_pending_and_returns_through_s30(tmp_path):
    """a function that is not an .amdhsa_kernel of its file is called with anything in flight; its return (s_setpc_b64 s[30:31]) ends it"""
    f = tmp_path / "k.s"
    f.write_text("""\t.type\t_Zhelper,@function
_Zhelper:
\ts_barrier ; BAD
\ts_waitcnt lgkmcnt(0)
\ts_barrier ; BAD
\ts_waitcnt vmcnt(0)
\ts_barrier
\ts_setpc_b64 s[30:31]
.Lfunc_end0:
\t.type\t_Zkernel,@function
_Zkernel:
\ts_barrier
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Zkernel
\t.end_amdhsa_kernel
\t.text
.Lfunc_end1:
""")
    got = {name: chk.check(body) for name, body in chk.kernels(str(f))}
    assert got == {"_Zhelper": [3, 5], "_Zkernel": []}
    ref = ref_functions(str(f))
    assert ref_check(ref["_Zhelper"], entry=3) == [3, 5] and ref_check(ref["_Zkernel"]) == []


def test_the_lds_dma_allow_list_excuses_only_the_dma_state_of_a_named_kernel(tmp_path, monkeypatch):
    text = """_Zkernel:
\tglobal_load_lds_dwordx4 v[2:3], off
\ts_waitcnt lgkmcnt(0)
\ts_barrier
\tds_write_b32 v1, v2
\ts_barrier
\ts_endpgm
.Lfunc_end0:
"""
    f = tmp_path / "k.s"
    f.write_text(text)
    (name, body), = list(chk.kernels(str(f)))
    assert chk.check(body) == [4, 6]
    monkeypatch.setitem(chk.DMA_ACROSS_BARRIER, "_Zkernel", "test: a three-buffer glds pipeline")
    assert chk.check(body) == [6]
    assert chk.DMA_ACROSS_BARRIER.keys() == {"_Zkernel"}
    monkeypatch.undo()
    assert chk.DMA_ACROSS_BARRIER == {}, "the library has no kernel that keeps an LDS-DMA in flight across a barrier"


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# differential fuzz: random functions in LLVM's textual shape, tool == reference on every one

STRAIGHT = [
    ("ds_write_b32 v1, v2 offset:16", 6), ("ds_write2_b64 v0, v[2:3], v[4:5] offset1:8", 2), ("ds_add_u32 v1, v2", 2), ("ds_cmpst_rtn_b32 v3, v1, v2, v4", 1),
    ("ds_read_b32 v3, v1", 4), ("ds_read2_b32 v[4:5], v1 offset1:1", 2), ("ds_bpermute_b32 v2, v1, v3", 2),
    ("global_load_lds_dwordx4 v[0:1], off", 3), ("buffer_load_dword v1, s[4:7], 0 offen lds", 1),
    ("s_waitcnt lgkmcnt(0)", 5), ("s_waitcnt lgkmcnt(1)", 3), ("s_waitcnt vmcnt(0)", 4), ("s_waitcnt vmcnt(2)", 3), ("s_waitcnt vmcnt(0) lgkmcnt(0)", 2),
    ("s_waitcnt vmcnt(2) lgkmcnt(0)", 1), (";;#ASMSTART\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND", 3),
    ("s_barrier", 8), ("v_add_u32_e32 v1, v2, v3", 3), ("s_mov_b32 s0, 0", 2), ("global_load_dword v1, v[2:3], off", 2), ("global_store_dword v[2:3], v1, off", 1),
    ("s_cmp_eq_u32 s0, 0", 2), ("s_swappc_b64 s[30:31], s[16:17]", 1), ("s_endpgm", 1),
]
BRANCHES = ["s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_execz", "s_cbranch_execnz", "s_cbranch_vccnz"]


def random_function(seed):
    """a function of 1-8 segments; a segment opens with a `.LBB` label or an unlabelled `; %bb.N:` and holds straight-line code with branches (forward and backward)
    and s_endpgm anywhere in it; the last instruction is s_endpgm or s_branch so that control never falls off the end"""
    rng = random.Random(seed)
    nseg = rng.randint(1, 8)
    labelled = [k == 0 or rng.random() < 0.6 for k in range(nseg)]
    labelled[0] = False
    targets = [f".LBB0_{k}" for k in range(nseg) if labelled[k]]
    pool, weights = zip(*STRAIGHT)
    out = ["\t.text", "\t.type\t_Zfuzz,@function", "_Zfuzz:                                 ; @_Zfuzz"]
    for k in range(nseg):
        out.append(f".LBB0_{k}:" + rng.choice(["", "                               ; =>This Inner Loop Header: Depth=1", "  ; %Flow"]) if labelled[k] else f"; %bb.{k}:")
        for _ in range(rng.randint(0, 12)):
            if targets and rng.random() < 0.12:
                out.append(f"\t{rng.choice(BRANCHES)} {rng.choice(targets)}")
            else:
                out.append("\t" + rng.choices(pool, weights)[0])
        if targets and rng.random() < 0.3:
            out.append(f"\t{rng.choice(BRANCHES)} {rng.choice(targets)}")
    out.append("\t" + (f"s_branch {rng.choice(targets)}" if targets and rng.random() < 0.3 else "s_endpgm"))
    out += ["\t.section\t.rodata,\"a\",@progbits", "\t.amdhsa_kernel _Zfuzz", "\t.end_amdhsa_kernel", "\t.text", ".Lfunc_end0:", ""]
    return "\n".join(out)


def test_the_tool_equals_the_reference_on_2000_random_functions(tmp_path):
    f = tmp_path / "fuzz.s"
    stats = {"flagged": 0, "clean_with_barriers": 0}
    for seed in range(2000):
        text = random_function(seed)
        f.write_text(text)
        (name, body), = list(chk.kernels(str(f)))
        want = ref_check(ref_functions(str(f))["_Zfuzz"])
        got = chk.check(body)
        assert got == want, f"seed {seed}: tool {got}, reference {want}\n{text}"
        stats["flagged"] += bool(want)
        stats["clean_with_barriers"] += not want and "s_barrier" in text
    assert min(stats.values()) >= 300, stats      # the generator exercises both outcomes


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the ISA of the build

@needs_isa
def test_the_tool_equals_the_reference_on_every_kernel_of_the_build():
    n = 0
    for path in isa_files():
        tool = {name: body for name, body in chk.kernels(path)}
        ref = ref_functions(path)
        assert tool.keys() == ref.keys(), (os.path.basename(path), sorted(tool.keys() ^ ref.keys()))
        for name, lines in ref.items():
            assert list(tool[name]) == lines, name
            assert chk.check(tool[name]) == ref_check(lines), name
            n += any(re.match(r"^\s+s_barrier", l) for _, l in lines)
    assert n >= 20, n


def _control(mnem):
    return re.match(r"^(s_branch|s_cbranch_\w+|s_endpgm\w*|s_setpc_b64|s_swappc_b64)$", mnem)


def mutants(body):
    """for every s_barrier: the body with every lgkmcnt(0) wait of the straight-line run before it deleted (a combined wait keeps its other fields)"""
    for k, (no, line) in enumerate(body):
        if not re.match(r"^\s+s_barrier\b", line):
            continue
        lines, changed, j = list(body), False, k - 1
        while j >= 0:
            s = lines[j][1].split(";")[0].strip()
            if re.fullmatch(r"[\w.$]+:", s) or (s and _control(s.split()[0])):
                break
            if s.startswith("s_waitcnt") and re.search(r"\blgkmcnt\(0\)", s):
                rest = re.sub(r"\s*\blgkmcnt\(0\)", "", s).strip()
                lines[j] = (lines[j][0], "\t" + rest if rest != "s_waitcnt" else "\t; (wait deleted)")
                changed = True
            j -= 1
        if changed:
            yield no, lines


@needs_isa
def test_every_barrier_that_loses_its_lds_waits_is_judged_like_the_reference():
    """the mutation: per s_barrier, delete the lgkmcnt(0) waits in front of it (the hard one of wg_barrier() and the compiler's soft one).  The tool must agree with the
    reference on every mutant, and catch the mid-block shape of k_lsd_gradient and of both production seed sorts (a label-only block split misses those)"""
    n, flagged_in = 0, {}
    for path in isa_files():
        for name, body in chk.kernels(path):
            for no, lines in mutants(list(body)):
                got, want = chk.check(lines), ref_check(lines)
                assert got == want, (name, no, got, want)
                n += 1
                if got:
                    flagged_in[name] = flagged_in.get(name, 0) + 1
    assert n >= 200, n
    assert sum(flagged_in.values()) >= 180, flagged_in
    for kernel in ("k_lsd_gradient", "ss_thr15k_lsd_seed_sort", "ss_lat15k_lsd_seed_sort"):
        assert any(kernel in name for name in flagged_in), (kernel, sorted(flagged_in))


@needs_isa
def test_every_declared_kernel_is_analysed_and_every_branch_target_resolves():
    for path in isa_files():
        text = open(path, errors="replace").read()
        declared = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
        found = {name: body for name, body in chk.kernels(path)}
        assert declared <= found.keys(), (os.path.basename(path), sorted(declared - found.keys()))
        for name, body in found.items():
            chk.check(body)                     # raises on a branch it cannot follow
            labels = {m.group(1) for _, l in body for m in [re.match(r"^\s*([\w.$]+):", l)] if m}
            for _, l in body:
                m = re.match(r"^\s+(s_branch|s_cbranch_\w+)\s+(\S+)", l)
                if m:
                    assert m.group(2) in labels, (name, l)


DS_WRITES = re.compile(r"^ds_(write|wrxchg|wrap|add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|cmpst|cmpswap|condxchg|pk_add|append|consume|gws|ordered)")


@needs_isa
def test_every_ds_mnemonic_of_the_build_is_classified():
    """each DS mnemonic the build uses is named here as a read or as a write, and the tool classifies it the same way; a new one fails this test until it is named"""
    seen = set()
    for path in isa_files():
        seen |= set(re.findall(r"^\s+(ds_\w+)", open(path, errors="replace").read(), re.M))
    assert seen
    for m in sorted(seen):
        is_read, is_write = m.startswith(READS), bool(DS_WRITES.match(m))
        assert is_read != is_write, f"{m}: not classified (or both)"
        assert chk.effect(m, "")[0] == (0 if is_read else chk.DS), m


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_compilers_own_glds_and_unmangled_kernel(tmp_path):
    """what hipcc makes of a glds before a barrier, in an extern "C" kernel: the raw s_barrier behind an lgkmcnt(0) wait is reached with the DMA in flight, the
    __syncthreads() path (whose fence waits vmcnt(0) while a glds is outstanding) is clean"""
    src = tmp_path / "g.hip"
    src.write_text("""#include <hip/hip_runtime.h>
extern "C" __global__ void k_glds(const int* __restrict__ in, int* out, int raw) {
    __shared__ int tile[256];
    const int t = threadIdx.x;
    __builtin_amdgcn_global_load_lds(in + blockIdx.x * 256 + t, &tile[0], 4, 0, 0);
    if (raw) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    } else {
        __syncthreads();
    }
    out[blockIdx.x * 256 + t] = tile[(t + 1) & 255];
}
""")
    out = tmp_path / "g.s"
    subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-mno-tgsplit", "--cuda-device-only", "-S", "-o", str(out), str(src)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    (name, body), = list(chk.kernels(str(out)))
    lines = open(out).read().split("\n")
    barriers = [no for no, l in body if re.match(r"^\s+s_barrier", l)]
    assert name == "k_glds" and len(barriers) == 2, (name, barriers)
    bad = chk.check(body)
    assert bad == ref_check(list(body)) and len(bad) == 1, bad
    before = [l.strip() for l in lines[:bad[0] - 1] if l.strip().startswith("s_waitcnt")]
    assert before[-1] == "s_waitcnt lgkmcnt(0)", before[-3:]
