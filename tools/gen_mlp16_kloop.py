#!/usr/bin/env python
"""Generator of the hand-scheduled k-loops of the large-row 16-bit MLP kernels (gaussianprediction_amd/csrc/deform_mlp16.hip).

    python tools/gen_mlp16_kloop.py            # rewrites gaussianprediction_amd/csrc/deform_mlp16_kloop.inc

One layer's product (K = 256: sixteen k-steps of v_mfma_f32_32x32x16) is ONE inline-asm statement with a fixed register
plan, because hipcc's version of the loop (a) waits for every LDS fragment right in front of the MFMA that reads it,
(b) prefetches the weight fragments one k-step deep behind `s_waitcnt vmcnt(0)`, and (c) has no registers left to carry
the saved-tensor stores of the tile the product is reading (round 4 / 5: the C++ attempts spilled inside the loop).

What the statement does per k-step (split mode, 64 rows x 64 features per wave, accumulators = operands):
  * 12 MFMAs:  am += Wh . Xh,  ax += Wl' . Xh,  ax += Wh . Xl'
  * the weight fragments of k-step ks + D (D = prefetch depth) requested from L2 (4 x 1 KB per wave),
  * the activation fragments of k-step ks + 1 read from LDS (4 x ds_read_b128),
  * CARRY: one 1 KB store of the tile being read (the saved tensor of the previous layer, blocked [16 rows][feature][16]):
    two ds_read_b64_tr_b16 (the LDS transpose read) gather 8 rows of one feature per lane, one global_store_dwordx4 writes them.
The waits are COUNTED: the generator keeps the two in-order queues (vmcnt: loads and stores together; lgkmcnt: LDS) and
emits, in front of every instruction, the largest count that still guarantees its operands -- never 0 inside the loop.

There is ONE path emitter (`emit_path`) and ONE statement frame (`statement`); the two forms (split fp16, plain 16-bit) are the
two `Form` records below and differ in data only.

Register plan (clobbered, fixed): see `Plan`.  Everything else (accumulators, addresses) are asm operands.
"""
import os
from dataclasses import dataclass
from typing import Callable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gaussianprediction_amd", "csrc", "deform_mlp16_kloop.inc")


class Queue:
    """An in-order completion counter (vmcnt or lgkmcnt): tags of the operations still outstanding, oldest first."""

    def __init__(self, name, limit):
        self.name, self.limit, self.q = name, limit, []

    def issue(self, tag):
        self.q.append(tag)
        assert len(self.q) <= self.limit, (self.name, len(self.q))

    def wait_for(self, tag):
        """Return the count to wait for so that every operation tagged `tag` has completed (None: already complete)."""
        idx = [i for i, t in enumerate(self.q) if t == tag]
        if not idx:
            return None
        n = len(self.q) - 1 - idx[-1]
        self.q = self.q[idx[-1] + 1:]
        return n

    def wait_all(self):
        if not self.q:
            return None
        self.q = []
        return 0


class Emitter:
    def __init__(self):
        self.lines = []
        self.vm = Queue("vmcnt", 63)
        self.lgkm = Queue("lgkmcnt", 15)

    def ins(self, s, head=""):
        """One line of the statement as C tokens: the string literal of the instruction `s`, behind the macro parameter `head` if given
        (adjacent literals concatenate, so the compiler sees one asm string)."""
        self.lines.append(f'{head} "{s}\\n\\t"'.lstrip())

    def need_vm(self, tag):
        n = self.vm.wait_for(tag)
        if n is not None:
            self.ins(f"s_waitcnt vmcnt({n})")

    def need_lgkm(self, tag):
        n = self.lgkm.wait_for(tag)
        if n is not None:
            self.ins(f"s_waitcnt lgkmcnt({n})")

    def define(self, name):
        """The lines as the body of the macro `name`."""
        return f"#define {name} \\\n" + " \\\n".join("    " + l for l in self.lines) + "\n"


def vr(base, n=1):
    return f"v{base}" if n == 1 else f"v[{base}:{base + n - 1}]"


class Plan:
    """Fixed VGPRs of one variant.  `first` is the lowest clobbered register."""

    def __init__(self, first, depth, n_b, n_a, carry):
        self.depth = depth
        self.n_b, self.n_a = n_b, n_a
        r = first
        self.B = r; r += 4 * n_b * (depth + 1)          # ring of depth + 1 weight-fragment groups
        self.A = r; r += 4 * n_a * 2                    # two activation-fragment groups
        self.ST = r; r += 4                             # the carried store's 16 bytes
        self.va = r; r += 1                             # LDS address of the activation fragments
        self.vw = r; r += 1                             # byte offset of the weight fragments / of the store
        self.t0 = r; r += 1                             # LDS addresses of the gather
        self.t1 = r; r += 1
        self.end = r
        self.first = first
        assert r <= 256, r

    def b(self, ks, q):
        return vr(self.B + 4 * (self.n_b * (ks % (self.depth + 1)) + q), 4)

    def a(self, ks, q):
        return vr(self.A + 4 * (self.n_a * (ks % 2) + q), 4)

    def clobbers(self):
        return ", ".join(f'"v{i}"' for i in range(self.first, self.end))


@dataclass(frozen=True)
class Form:
    """What distinguishes one form of the product from the other: data only, read by `emit_path` and `statement`."""
    name: str
    mn: str                 # the MFMA mnemonic, or
    args: str               # "(MN)": `mn` names the macro parameter that stands for it in every macro of the form
    depth: int              # prefetch depth of the weight fragments, in k-steps
    b_bases: tuple          # scalar base of each weight fragment of a k-step (1 KB each; odd fragments at offset:1024 of their base)
    a_off: tuple            # LDS byte offsets of the four activation fragments of a k-step
    seq: Callable           # (ks, init) -> [(accumulator, weight fragment, activation fragment, addend or None = the accumulator)]
    slots: dict             # behind which MFMA of a k-step each side operation is issued
    gather_lit: Callable    # (g, pass) -> XOR literal of the transpose read's address
    gather_off: Callable    # (g, pass) -> its offset

    def plan(self):
        n_b, n_a = len(self.b_bases), len(self.a_off)
        return Plan(256 - (4 * n_b * (self.depth + 1) + 8 * n_a + 8), self.depth, n_b, n_a, True)


# The bias enters as an ADDEND: with init = "bias" the accumulators of row tile 0 hold the bias on entry (every row tile starts from
# the same 32 features' biases), the first MFMA of every other row tile reads them as its addend, and row tile 0 goes last in k-step 0,
# BEFORE which nothing overwrites it -- so no accumulator is ever initialised by VALU moves.  init = "zero": nothing is read on
# entry; every first MFMA takes the inline constant 0.
def split_seq(ks, init):
    """Split fp16, 64-row workgroup: 2 row tiles x 2 feature tiles per wave, hi x hi (am) first, then the two cross terms (ax), which
    always start from 0.  Weight fragments 0 1 = Wh, 2 3 = Wl'; activation fragments 0 2 = Xh, 1 3 = Xl' of row tiles 0 1."""
    seq = [("am00", 0, 0, None), ("am01", 1, 0, None), ("am10", 0, 2, None), ("am11", 1, 2, None),
           ("ax00", 2, 0, None), ("ax01", 3, 0, None), ("ax10", 2, 2, None), ("ax11", 3, 2, None),
           ("ax00", 0, 1, None), ("ax01", 1, 1, None), ("ax10", 0, 3, None), ("ax11", 1, 3, None)]
    if ks == 0:
        if init == "bias":
            seq[0:4] = [("am10", 0, 2, "%[am00]"), ("am11", 1, 2, "%[am01]"), ("am00", 0, 0, None), ("am01", 1, 0, None)]
        else:
            seq[0:4] = [(a, b, c, "0") for a, b, c, _ in seq[0:4]]
        seq[4:8] = [(a, b, c, "0") for a, b, c, _ in seq[4:8]]
    return seq


def plain_seq(ks, init):
    """Plain 16-bit (fp16 / bf16 operands), 128-row workgroup: 4 row tiles x 2 feature tiles per wave = 8 accumulators c<rt><nt>,
    8 MFMAs per k-step from two weight fragments and four activation fragments (one per row tile)."""
    order = [1, 2, 3, 0] if ks == 0 and init == "bias" else [0, 1, 2, 3]
    seq = []
    for rt in order:
        for nt in range(2):
            src = None
            if ks == 0:
                src = "0" if init == "zero" else (f"%[c0{nt}]" if rt else None)
            seq.append((f"c{rt}{nt}", nt, rt, src))
    return seq


# The carried store: wave w owns 16-row blocks of the tile being read; k-step g writes 32 features of one block, g KB into the wave's
# part of the saved tensor.  Split (rows of 1024 bytes, block w): features 32 g .. + 31 of [hi | lo'].  Plain (rows of 512 bytes,
# blocks 2 w and 2 w + 1): features 32 (g & 7) .. + 31 of block 2 w + (g >> 3).
SPLIT = Form(name="M16S", mn="v_mfma_f32_32x32x16_f16", args="", depth=3,
             b_bases=("%[swh]", "%[swh]", "%[swl]", "%[swl]"),
             a_off=(0, 512, 32768, 33280),                                    # ah rt0, al' rt0, ah rt1, al' rt1
             seq=split_seq, slots=dict(load=0, gather=(1, 2), read=(5, 6), store=9),
             gather_lit=lambda g, ps: 64 * (g ^ ps), gather_off=lambda g, ps: 4096 * ps)
PLAIN = Form(name="M16P", mn="MN", args="(MN)", depth=5,
             b_bases=("%[swh]", "%[swh]"),
             a_off=(0, 16384, 32768, 49152),                                  # rt0 .. rt3
             seq=plain_seq, slots=dict(load=0, gather=(1, 2), read=(3, 4), store=6),
             gather_lit=lambda g, ps: 64 * ((g & 7) ^ ps), gather_off=lambda g, ps: 2048 * ps + 8192 * (g >> 3))


def emit_path(f, p, nks, carry, init):
    """One product (nks k-steps) of the form `f` on the register plan `p`, as a fresh Emitter: a path starts and ends with both
    queues empty as far as anything behind it is concerned, so paths do not depend on each other."""
    e = Emitter()
    KST = 8192                                        # bytes per k-step of the fragment-packed weights (8 feature tiles x 1 KB)

    def load_b(ks):
        if ks == 0:
            off = "%[voff]"
        else:
            e.ins(f"v_add_u32 {vr(p.vw)}, {ks * KST}, %[voff]")
            off = vr(p.vw)
        for q, base in enumerate(f.b_bases):
            e.ins(f"global_load_dwordx4 {p.b(ks, q)}, {off}, {base}" + (" offset:1024" if q & 1 else ""))
            e.vm.issue(("B", ks))

    def read_a(ks, qs):
        if qs[0] == 0:
            if ks == 0:
                e.ins(f"v_mov_b32 {vr(p.va)}, %[abase]")
            else:
                e.ins(f"v_xor_b32 {vr(p.va)}, {ks * 32}, %[abase]")
        for q in qs:
            e.ins(f"ds_read_b128 {p.a(ks, q)}, {vr(p.va)}" + (f" offset:{f.a_off[q]}" if f.a_off[q] else ""))
            e.lgkm.issue(("A", ks, q))

    def gather(g, ps):
        # ds_read_b64_tr_b16 = every lane reads 8 bytes at ITS address, then lane l of a 16-lane group receives element (l & 3) of lanes
        # (l >> 2), 4 + (l >> 2), 8 + (l >> 2), 12 + (l >> 2) (measured: tools/probe/ds_tr_probe.hip).  Lane 4 j + q of a group
        # reads features 4 q .. 4 q + 3 of row j, so lane l receives rows 0 .. 3 of feature l: the 4 x 16 transpose in one
        # instruction; two passes (rows 0-3, 4-7) make the 16 bytes of the blocked layout.  (The d16 sub-dword loads cannot build it:
        # with SRAM-ECC a d16 load zeroes the other half of the register.)
        t = vr(p.t0 if ps == 0 else p.t1)
        lit, off = f.gather_lit(g, ps), f.gather_off(g, ps)
        if lit:
            e.ins(f"v_xor_b32 {t}, {lit}, %[sbt]")
            src = t
        else:
            src = "%[sbt]"
        e.ins(f"ds_read_b64_tr_b16 {vr(p.ST + 2 * ps, 2)}, {src}" + (f" offset:{off}" if off else ""))
        e.lgkm.issue(("G", g))

    def store(g):
        e.need_lgkm(("G", g))
        if g == 0:
            off = "%[vost]"
        else:
            e.ins(f"v_add_u32 {vr(p.vw)}, {g * 1024}, %[vost]")
            off = vr(p.vw)
        e.ins(f"global_store_dwordx4 {off}, {vr(p.ST, 4)}, %[sst]")
        e.vm.issue(("S", g))

    def mfma(acc, ks, bq, aq, src=None):
        e.need_vm(("B", ks))
        e.need_lgkm(("A", ks, aq))
        ops = f" %[{acc}], {p.b(ks, bq)}, {p.a(ks, aq)}, {src if src is not None else '%[' + acc + ']'}"
        if f.args:
            e.ins(ops, head=f.mn)
        else:
            e.ins(f.mn + ops)

    # prologue: the first `depth` weight groups and the first activation group
    for ks in range(min(f.depth, nks)):
        load_b(ks)
    read_a(0, [0, 1, 2, 3])
    s = f.slots
    for ks in range(nks):
        for m, (acc, bq, aq, src) in enumerate(f.seq(ks, init)):
            mfma(acc, ks, bq, aq, src)
            # the slots behind the MFMAs (the matrix pipe is busy for 32 cycles per MFMA: anything here issues for free)
            if m == s["load"] and ks + f.depth < nks:
                load_b(ks + f.depth)
            if carry and m in s["gather"]:
                gather(ks, s["gather"].index(m))
            if m in s["read"] and ks + 1 < nks:
                read_a(ks + 1, [[0, 1], [2, 3]][s["read"].index(m)])
            if carry and m == s["store"]:
                store(ks)
    assert not e.lgkm.q, e.lgkm.q
    e.vm.q = []                 # (stores may still be in flight at the end of a path: nothing below depends on the count)
    return e


def statement(first, second):
    """One asm statement = one product with two PATHS (macros of their own, so that a path shared by several statements is written
    once) selected by the scalar operand `sel` (0 = the first path): the K = 256 layers, and the layer with its own k-step count
    (forward: layer 0, K = in_pad; data backward: the output layer, K = 16).  Both paths use the same operands and registers, so the
    layer loop around the statement is one rolled loop with ONE statement in it -- with several statements (or the compiler's loop
    beside it) hipcc assigned the 128 accumulator registers differently per path and moved them between the paths (240 v_mov per
    layer).
    Operands: the accumulators (f32x16; split: am00 am01 am10 am11 ax00 ax01 ax10 ax11, plain: c00 .. c31), abase (LDS byte address of
    this lane's row, swizzle folded in), voff (lane * 16), swh and, split only, swl (SGPR pairs: this wave's hi / lo' weight
    fragments), sel, and for a carrying path sbt (LDS byte address this lane supplies to the transpose reads), vost (this lane's byte
    offset in a 1 KB chunk of the saved tensor) and sst (SGPR pair: this wave's part of the saved tensor)."""
    e = Emitter()
    e.ins("s_cmp_eq_u32 %[sel], 0")
    e.ins("s_cbranch_scc0 71f")
    e.lines.append(first)
    e.ins("s_branch 72f")
    e.ins("71:")
    e.lines.append(second)
    e.ins("72:")
    # the accumulators are read by VALU code right behind this statement: XDL write -> VALU read needs passes + 3 wait states
    e.ins("s_nop 15")
    return e


HEADER = """// GENERATED by tools/gen_mlp16_kloop.py -- do not edit.  The hand-scheduled k-loops of the large-row 16-bit MLP kernels:
// one inline-asm statement per layer product (<form>_<product>_ASM), composed of two paths (<form>_K<k-steps>[_CARRY]_<init>_PATH,
// each distinct path once).  One emitter in the generator, the forms (M16S: split fp16, M16P: plain 16-bit) described by a table;
// the plain macros are parameterised by the MFMA mnemonic: M16P_FWD_TRAIN_ASM("v_mfma_f32_32x32x16_bf16").  Register plan, counted
// waits and the carried saved-tensor stores are described in the generator.
"""

# (product, [(k-steps, carry) of the first path, of the second path], init)
STATEMENTS = (("FWD_TRAIN", [(16, True), (7, False)], "bias"), ("FWD_INFER", [(16, False), (7, False)], "bias"),
              ("BWD_DATA", [(16, True), (1, False)], "zero"))


def render():
    """The whole text of the .inc."""
    parts = [HEADER]
    for f in (SPLIT, PLAIN):
        p = f.plan()
        defined = set()
        for product, paths, init in STATEMENTS:
            names = []
            for nks, carry in paths:
                names.append(f"{f.name}_K{nks}{'_CARRY' if carry else ''}_{init.upper()}_PATH{f.args}")
                if names[-1] not in defined:
                    defined.add(names[-1])
                    parts.append(emit_path(f, p, nks, carry, init).define(names[-1]))
            parts.append(statement(*names).define(f"{f.name}_{product}_ASM{f.args}"))
        parts.append(f"#define {f.name}_KLOOP_CLOBBERS {p.clobbers()}\n")
    return "\n".join(parts)


def main():
    with open(OUT, "w") as f:
        f.write(render())
    print("wrote", OUT)


if __name__ == "__main__":
    main()

