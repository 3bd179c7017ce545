"""The fused backward kernels keep their output stores in flight across tiles (host test: needs hipcc, no GPU).

A persistent workgroup requests tile i + 1 before the products of tile i and stores tile i's gradient after them.  vmcnt
retires in issue order, so a wait for vmcnt(0) inside the tile loop waits for the acknowledgement of stores that are
YOUNGER than the loads it is there for: the matrix pipe idles for a round trip to HBM per tile.  With every load and store
issued unconditionally (buffer descriptors, empty when there is nothing to fetch) the number of operations behind a request
is static and the compiler emits a counted wait instead.

For each kernel below the assembly hipcc produces for gfx950 is searched: inside the outermost loop that holds matrix
instructions there is no `s_waitcnt vmcnt(0)`, and the kernel has no scratch instruction anywhere.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamorph_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")

# file -> substrings of the demangled kernel names the rule is checked on (every instantiation the C3 step or C5 runs)
KERNELS = {
    "convT_bwd.hip": ["convT_bwd_kernel<16, 8, 16>", "convT_bwd_kernel<8, 4, 32>"],
    "conv4x4s2_patch.hip": ["conv4x4s2_bwd_kernel", "conv4x4s2_patch_forward_kernel"],
    "conv3x3_bwd.hip": ["conv3x3_bwd_counted_kernel<32, 512>", "conv3x3_bwd_kernel<16, 256, false>", "conv3x3_bwd_kernel<32, 512, true>"],
    "conv1x1_bwd.hip": ["conv1x1_bwd_kernel"],
}
# kernel-name substring -> (full drains it keeps inside its tile loop, why).  No scratch holds for these too.
EXCEPTIONS = {
    "conv3x3_bwd_kernel<16, 256, false>": (3, "left as it was: at its commit and in front of the dx stores of each of its two row pairs.  Holding the "
                                              "side inputs (residual, statistics partner) in flight across the products takes more than the 256 "
                                              "registers a wave has (56 bytes of scratch); with the commit alone counted it measured 55.2 us "
                                              "against 54.8"),
    "conv3x3_bwd_kernel<32, 512, true>": (1, "left as it was (C5 only): in front of the dx stores of its row pair, for the same reason (64 bytes of "
                                             "scratch); its commit waits by hand for all but the stores"),
    "conv1x1_bwd_kernel": (1, "not touched by this rule's change: its commit waits for the x tile, requested last, with vmcnt(0)"),
}

_asm_cache = {}


def _assembly(src):
    """{demangled kernel name: [instruction lines]} of one source file."""
    if src in _asm_cache:
        return _asm_cache[src]
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
           "-S", os.path.join(CSRC, src), "-o", "-"]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=CSRC).stdout
    bodies, name, lines = {}, None, []
    for ln in text.splitlines():
        mm = re.match(r"^(_Z\w+):", ln)
        if mm and name is None:
            name, lines = mm.group(1), []
        elif name is not None:
            if ln.strip().startswith(".Lfunc_end"):
                bodies[name] = lines
                name = None
            else:
                lines.append(ln.split(";")[0].rstrip())
    filt = shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    names = list(bodies)
    dem = subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
    out = {d.replace("(anonymous namespace)::", ""): bodies[n] for n, d in zip(names, dem)}
    _asm_cache[src] = out
    return out


def _blocks(lines):
    """Basic blocks [(first, last)] of a kernel body and their successors (indices into the block list)."""
    label_at = {}
    starts = {0}
    for i, ln in enumerate(lines):
        mm = re.match(r"^(\.LBB\w+):", ln)
        if mm:
            label_at[mm.group(1)] = i
            starts.add(i)
        elif re.match(r"^\s+(s_c?branch\w*|s_endpgm)\b", ln):
            starts.add(i + 1)
    starts = sorted(x for x in starts if x < len(lines))
    blocks = [(a, (starts[k + 1] if k + 1 < len(starts) else len(lines)) - 1) for k, a in enumerate(starts)]
    index_of = {a: k for k, (a, _) in enumerate(blocks)}
    succ = []
    for k, (a, z) in enumerate(blocks):
        last = next((lines[i] for i in range(z, a - 1, -1) if lines[i].strip() and not lines[i].lstrip().startswith(".")), "")
        mm = re.match(r"^\s+(s_c?branch\w*)\s+(\.LBB\w+)", last)
        out = []
        if mm:
            out.append(index_of[label_at[mm.group(2)]])
        if not (mm and mm.group(1) == "s_branch") and "s_endpgm" not in last and k + 1 < len(blocks):
            out.append(k + 1)
        succ.append(out)
    return blocks, succ


def _tile_loop(lines):
    """Line ranges of the blocks of the outermost loop that holds matrix instructions: the strongly connected component of the
    control-flow graph they are in (a block laid out behind the loop that is only entered from the prologue is not part of it)."""
    blocks, succ = _blocks(lines)
    n = len(blocks)
    reach = []
    for k in range(n):                                           # (a few hundred blocks: plain reachability is enough)
        seen, todo = set(), list(succ[k])
        while todo:
            j = todo.pop()
            if j not in seen:
                seen.add(j)
                todo.extend(succ[j])
        reach.append(seen)
    mf = [k for k, (a, z) in enumerate(blocks) if any("v_mfma" in x for x in lines[a:z + 1]) and k in reach[k]]
    assert mf, "no loop with matrix instructions found"
    comp = {k for k in range(n) if k in reach[mf[0]] and mf[0] in reach[k]}
    assert all(k in comp for k in mf), "matrix instructions in more than one loop nest"
    return [blocks[k] for k in sorted(comp)]


def _check(src, kernel):
    found = [(n, b) for n, b in _assembly(src).items() if kernel in n]
    assert found, f"{kernel}: not in the assembly of {src}"
    drains, scratch = [], []
    for name, lines in found:
        scratch += [f"{name}: {ln.strip()}" for ln in lines if re.match(r"^\s+scratch_", ln)]
        for a, z in _tile_loop(lines):
            drains += [f"{name}: line {i} of the kernel" for i in range(a, z + 1) if re.match(r"^\s+s_waitcnt\b.*vmcnt\(0\)", lines[i])]
    return drains, scratch


@pytest.mark.parametrize("src,kernel", [(s, k) for s, ks in KERNELS.items() for k in ks])
def test_no_store_drain_inside_the_tile_loop(src, kernel):
    drains, scratch = _check(src, kernel)
    assert not scratch, f"{len(scratch)} scratch instructions, e.g. {scratch[0]}"
    allowed = next((n for k, (n, _) in EXCEPTIONS.items() if k in kernel), 0)
    assert len(drains) <= allowed, f"{len(drains)} x s_waitcnt vmcnt(0) inside the tile loop ({allowed} allowed):\n" + "\n".join(drains)
