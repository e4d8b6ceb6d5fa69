#!/usr/bin/env python3
"""Every s_barrier of every kernel must be reached with the wave's own LDS writes drained, on every path through the kernel's ISA.

Why this exists (profiles/r06_seed_sort.md section 4): `__syncthreads()` is a workgroup release fence + s_barrier, and the fence's `s_waitcnt lgkmcnt(0)` is a SOFT wait the
compiler's wait-count pass may drop where its scoreboard shows no LDS operation pending.  In a diagnostic build of the seed sort it dropped the wait at the barrier that heads
the loop over a frame's global partitions -- on the path from the kernel's entry nothing is pending there, on the back edge wave 0's pushes to the segment stack are -- and
the other waves then read the stack before wave 0's writes had landed: the "failure beside a second dispatch" of rounds 4 - 6.  The library's barriers carry a hard wait
(csrc/plp_barrier.hpp); this tool reads the ISA the build keeps (csrc/build/*.s) and checks it per function by a forward data-flow over its basic blocks.

What a clean result establishes, and under which assumptions:
  * Two pending states per wave.  A DS write or atomic (every `ds_*` except the read-only set below) is pending until an `s_waitcnt` with lgkmcnt(0).  An LDS-DMA
    (`global_load_lds_*`, `buffer_load_* ... lds`: a load that writes LDS, counted on the VM counter) is pending until an `s_waitcnt` with vmcnt(0); a counted vmcnt(N > 0)
    does not drain it.  A FLAT / scratch store or atomic may reach LDS and is counted on both counters: it sets both states.  An s_barrier reached on ANY path with either
    state set is reported -- unless its kernel is on DMA_ACROSS_BARRIER below, which only excuses the LDS-DMA state.
  * Blocks end at every label and after every s_branch, s_cbranch_*, s_endpgm, s_setpc_b64 and s_swappc_b64, so a conditional branch carries the state at the branch.
  * Calls are conservative: after an `s_swappc_b64` both states are pending (the callee may write LDS), and a function that is not a kernel is entered with both pending.
  * Unknown control flow is an error (ValueError), never a fall-through: a branch to a label that is not in the same function, `s_setpc_b64` other than a non-kernel function's
    return through s[30:31], `s_cbranch_g_fork` / `s_cbranch_join` / `s_rfe_*` / `s_call_*`, code falling off the end of a function, a directive that may emit code inside one,
    and an `s_waitcnt` whose operand cannot be read.
  * Unreachable code is analysed as if entered with nothing pending.
Not established: whether a barrier that hands data from wave to wave through HBM needs vmcnt(0) for the wave's GLOBAL stores (wg_barrier_after_global_stores() in
csrc/plp_barrier.hpp) -- which barriers need that depends on what the code means, not on the ISA alone.  The check also trusts the assembler's text: it reads what the compiler
printed, not the code object.

    python tools/isa_barrier_check.py [file.s ...]      (default: structure-plp-slam_amd/csrc/build/*.s)      exit code 1 = some barrier can be reached with LDS writes in flight
"""
import glob, os, re, sys

DS, DMA = 1, 2          # the two pending states: a DS write (lgkmcnt), an LDS-DMA (vmcnt)

# Kernels that keep an LDS-DMA in flight across a barrier ON PURPOSE (a multi-buffered glds pipeline that retires each buffer with a counted vmcnt(N) before the barrier
# that precedes its read).  name -> the reason, in a comment-sized sentence.  Only the DMA state is excused; a DS write
# in flight at a barrier is still reported.  This library has no such kernel.
DMA_ACROSS_BARRIER = {}

TYPE_FUNC = re.compile(r"^\s*\.type\s+([^\s,]+)\s*,\s*@function\b")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LABEL = re.compile(r"^\s*([A-Za-z_.$][\w.$]*):(.*)$")
DS_READ_ONLY = ("ds_read", "ds_bpermute", "ds_permute", "ds_swizzle", "ds_nop")
# directives that only place or annotate code; any other directive inside a function may emit bytes the check cannot see, and is an error
QUIET_DIRECTIVES = re.compile(r"^\.(p2align|balign|align|loc|file|cfi_\w+)\b")
WAIT_FIELD = re.compile(r"^(vmcnt|expcnt|lgkmcnt)(?:_sat)?\((\d+)\)$")


class Body(list):
    """the (line number, text) lines of one function, with its name and whether the file declares it a kernel (.amdhsa_kernel)"""
    def __init__(self, lines=(), name=None, kernel=True):
        super().__init__(lines)
        self.name, self.kernel = name, kernel


def kernels(path):
    """yield (name, Body) for every function of an assembly file: `.type sym,@function`, then `sym:` ... `.Lfunc_end*:`.  In a listing without any `.type` directive (a
    hand-written or cut-down one) every column-0 label that is not local (.L*) opens a function, and a file that declares no `.amdhsa_kernel` holds kernels only.  A function that
    is never closed, or an `.amdhsa_kernel` whose code was not found, is an error."""
    lines = open(path, errors="replace").read().split("\n")
    funcs = {m.group(1) for m in map(TYPE_FUNC.match, lines) if m}
    typed = any(re.match(r"^\s*\.type\s", line) for line in lines)
    declared_kernels = {m.group(1) for m in map(KERNEL.match, lines) if m}
    name, body, found = None, None, set()
    for no, line in enumerate(lines, 1):
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w.$]*):", line)
            if m and (not typed or m.group(1) in funcs):
                name = m.group(1)
                body = Body(name=name, kernel=not declared_kernels or name in declared_kernels)
        elif line.startswith(".Lfunc_end"):
            found.add(name)
            yield name, body
            name = None
        else:
            body.append((no, line))
    if name is not None:
        raise ValueError(f"{path}: function {name} has no .Lfunc_end")
    if declared_kernels - found:
        raise ValueError(f"{path}: .amdhsa_kernel without a function body: {sorted(declared_kernels - found)}")


def waitcnt(operands):
    """(vmcnt, lgkmcnt) an s_waitcnt waits for; None = that counter is not waited for"""
    ops = operands.strip()
    if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", ops):           # the raw simm16 of gfx9: vmcnt bits 3:0 and 15:14, lgkmcnt bits 11:8
        v = int(ops, 0)
        return (v & 0xF) | ((v >> 10) & 0x30), (v >> 8) & 0xF
    fields = [WAIT_FIELD.match(tok) for tok in re.split(r"[\s,&]+", ops) if tok]
    if not fields or not all(fields):
        raise ValueError(f"cannot read s_waitcnt operand {operands!r}")
    got = {m.group(1): int(m.group(2)) for m in fields}
    return got.get("vmcnt"), got.get("lgkmcnt")


def effect(mnem, ops):
    """the pending states an instruction sets: (set bits, cleared bits)"""
    if mnem == "s_waitcnt":
        vm, lgkm = waitcnt(ops)
        return 0, (DS if lgkm == 0 else 0) | (DMA if vm == 0 else 0)
    vmem = mnem.startswith(("buffer_", "tbuffer_", "global_", "flat_", "scratch_"))
    if vmem and ("_lds" in mnem or "lds" in re.split(r"[\s,]+", ops)):
        return DMA, 0
    if mnem.startswith("ds_") and not mnem.startswith(DS_READ_ONLY):
        return DS, 0
    if mnem.startswith(("flat_store", "flat_atomic", "scratch_store", "scratch_atomic")):
        return DS | DMA, 0
    if mnem == "s_swappc_b64":
        return DS | DMA, 0
    return 0, 0


def instructions(body):
    """[(line_no, label or None, mnemonic or None, operands)] of the function's code, with comments dropped; a label gives (no, label, None, '').  What lies in another
    section between the function's label and its end (LLVM places the .amdhsa_kernel descriptor there, in .rodata) is not code and is skipped."""
    out, in_text = [], True
    for no, line in body:
        text = re.split(r";|//", line, maxsplit=1)[0].strip()
        m = re.match(r"^\.(section|text|data|bss|rodata|pushsection|popsection|previous|subsection)\b\s*([^\s,]*)", text)
        if m:
            if m.group(1) in ("pushsection", "popsection", "previous", "subsection"):
                raise ValueError(f"line {no}: section stack inside a function: {text!r}")
            in_text = m.group(1) == "text" or (m.group(1) == "section" and m.group(2).startswith(".text"))
            continue
        while text and in_text:
            m = LABEL.match(text)
            if m:
                out.append((no, m.group(1), None, ""))
                text = m.group(2).strip()
                continue
            if text.startswith("."):
                if not QUIET_DIRECTIVES.match(text):
                    raise ValueError(f"line {no}: directive inside a function: {text!r}")
                break
            mnem, ops = (re.split(r"\s+", text, maxsplit=1) + [""])[:2]
            out.append((no, None, mnem, ops))
            break
    return out


def control(mnem, ops, kernel, labels, no):
    """(branch target or None, falls through) of one instruction; raises on control flow it cannot follow"""
    if mnem in ("s_cbranch_g_fork", "s_cbranch_join") or mnem.startswith(("s_rfe", "s_call")):
        raise ValueError(f"line {no}: unsupported control flow {mnem}")
    if mnem == "s_branch" or mnem.startswith("s_cbranch_"):
        target = ops.split(",")[0].strip()
        if target not in labels:
            raise ValueError(f"line {no}: {mnem} to {target!r}, which is not a label of this function")
        return target, mnem != "s_branch"
    if mnem.startswith("s_endpgm"):
        return None, False
    if mnem == "s_setpc_b64":
        if kernel or ops.replace(" ", "") != "s[30:31]":
            raise ValueError(f"line {no}: s_setpc_b64 {ops} is an indirect jump, not a return")
        return None, False
    return None, True


# (s_rfe / s_call end a block only to reach control(), which refuses them)
ENDS_BLOCK = re.compile(r"^(s_branch|s_cbranch_\w+|s_endpgm\w*|s_setpc_b64|s_swappc_b64|s_rfe\w*|s_call\w*)$")


def check(body):
    """basic blocks, successors, then the data-flow over the two pending states; returns the sorted line numbers of barriers reached with a state pending"""
    kernel = getattr(body, "kernel", True)
    excused = DMA if getattr(body, "name", None) in DMA_ACROSS_BARRIER else 0
    ins = instructions(body)
    labels = {lab for _, lab, _, _ in ins if lab}
    blocks, index, cur = [], {}, None
    for no, lab, mnem, ops in ins:
        if lab:
            if lab in index:
                raise ValueError(f"line {no}: label {lab} defined twice")
            cur = {"ins": [], "succ": [], "falls": True}
            blocks.append(cur)
            index[lab] = len(blocks) - 1
            continue
        if cur is None:
            cur = {"ins": [], "succ": [], "falls": True}
            blocks.append(cur)
        cur["ins"].append((no, mnem, ops))
        if ENDS_BLOCK.match(mnem):
            cur = None
    for i, b in enumerate(blocks):
        if b["ins"]:
            no, mnem, ops = b["ins"][-1]
            target, b["falls"] = control(mnem, ops, kernel, labels, no)
            if target:
                b["succ"].append(index[target])
        if b["falls"]:
            if i + 1 == len(blocks):
                raise ValueError(f"control falls off the end of {getattr(body, 'name', None) or 'the function'}")
            b["succ"].append(i + 1)
    if not blocks:
        return []
    # every block is visited once from the empty state (the entry from its own); a block is visited again whenever a predecessor adds a pending state to its input
    state_in = [0] * len(blocks)
    state_in[0] = 0 if kernel else DS | DMA
    seen = [None] * len(blocks)
    work, bad = list(range(len(blocks)))[::-1], set()
    while work:
        i = work.pop()
        st = state_in[i]
        if seen[i] == st:
            continue
        seen[i] = st
        for no, mnem, ops in blocks[i]["ins"]:
            if mnem.startswith("s_barrier") and st & ~excused:
                bad.add(no)
            on, off = effect(mnem, ops)
            st = (st & ~off) | on
        for j in blocks[i]["succ"]:
            if state_in[j] | st != state_in[j]:
                state_in[j] |= st
                work.append(j)
    return sorted(bad)


def main(paths):
    rc = 0
    for path in paths:
        for name, body in kernels(path):
            try:
                n_bar = sum(1 for _, _, mnem, _ in instructions(body) if mnem and mnem.startswith("s_barrier"))
                bad = check(body)
            except ValueError as e:
                print(f"{os.path.basename(path)}: {name[:70]:70s} CANNOT BE CHECKED: {e}")
                rc = 1
                continue
            if not n_bar:
                continue
            print(f"{os.path.basename(path)}: {name[:70]:70s} barriers {n_bar:3d}  reached with LDS writes in flight: {len(bad)}" + (f"  (lines {bad[:8]})" if bad else ""))
            rc |= bool(bad)
    return rc


if __name__ == "__main__":
    args = sys.argv[1:] or sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "structure-plp-slam_amd", "csrc", "build", "*.s")))
    sys.exit(main(args))
