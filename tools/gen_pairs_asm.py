#!/usr/bin/env python3
"""Writes spandsp_amd/csrc/tone_pairs_asm.inc: the sixteen sample pairs of one 64-byte row piece as ONE inline-asm body,
in these forms (tone_fast.hpp): SPG_PAIRS_ASM_* can be entered at any pair and left after any pair (the segment that holds a
block end, as it was first built: a read and an exit test per pair); SPG_PAIRS_COMMON_ASM_* is the sixteen pair blocks straight
through, with no entry tree and no exit tests, its samples fetched by four ds_read_b128 up front and waited for chunk by chunk
(the common segment); SPG_PAIRS_HEAD_ASM_* and SPG_PAIRS_TAIL_ASM_* are that common body left after a pair and entered at a
pair (the two halves of the segment that holds a block end, as the library builds it; not in the v_pk_fma_f32 file).  Written in C++ the
energy's squares and adds are pure operations that instruction selection sinks behind the last asm statement of the
recurrence, one serial chain of thirty-two adds at the end of the segment (profiles/tone_energy_in_gaps.md); here they sit
in the issue slots the recurrence leaves.

Why generated: every pair block differs from its neighbours only in constants (which LDS dword it converts, which dword is
requested three pairs ahead, how many LDS reads may still be on their way), and the body exists for every number of packed
bin pairs a detector has (NP) with and without the block energy.  The arithmetic of a pair is Bank<>::step2's: per bin pair
v_pk_mul_f32, v_pk_add_f32 (neg), v_pk_add_f32 with op_sel picking the sample -- (fac*v2 - v1) + x rounded three times, as
src/spandsp/tone_detect.h:172-192 does -- and energy += x*x per sample in sample order (src/dtmf.c:199).

Fixed registers (clobbered): T_i = v[100+2i:101+2i] (i < 4), X = v[108:109], SQ = v[110:111], D0..D3 = v112..v115
(as low as the kernel's own register use allows: the highest one sets the wave's allocation); the common body's four chunks
are v[112:127], pair k's dword in v(112 + k) -- and, once converted, the samples of an odd pair.
A packed result must not be read by the very next instruction (one wait state on gfx950): the order below keeps every
reader of a 64-bit result at least one instruction away.
"""
import os

OUT = os.path.join(os.path.dirname(__file__), "..", "spandsp_amd", "csrc", "tone_pairs_asm.inc")


def T(i):
    return "v[%d:%d]" % (100 + 2*i, 101 + 2*i)


X = "v[108:109]"
XL, XH = "v108", "v109"
SQ = "v[110:111]"
SQL, SQH = "v110", "v111"


def D(k):
    return "v%d" % (112 + (k % 4))


def read(k):
    return "ds_read_b32 %s, %%[ad%d] offset:%d" % (D(k), k//4, 4*(k % 4))


def pair_block(L, np_, energy, fma, d):
    """One sample pair, its dword in register d: the two converts, the recurrence, and (energy) the squares as one packed
    product and the two adds in sample order, neither next to the other nor directly behind the product."""
    a = lambda i: "%%[a%d]" % i
    b = lambda i: "%%[b%d]" % i
    f = lambda i: "%%[f%d]" % i
    L.append("v_cvt_f32_i32_sdwa %s, sext(%s) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" % (XL, d))
    L.append("v_cvt_f32_i32_sdwa %s, sext(%s) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" % (XH, d))
    if fma:
        # the experiment of round 6 (-DSPG_TONE_FMA, NOT bit-exact): fac*v2 - v1 as ONE v_pk_fma_f32 -- 2 packed operations
        # per bin pair and sample in place of 3 -- then + x as before
        L += ["v_pk_fma_f32 %s, %s, %s, %s neg_lo:[0,0,1] neg_hi:[0,0,1]" % (T(i), f(i), b(i), a(i)) for i in range(np_)]
        if energy:
            L.append("v_pk_mul_f32 %s, %s, %s" % (SQ, X, X))
        if np_ == 1:
            L.append("s_nop 0")
        L += ["v_pk_add_f32 %s, %s, %s op_sel_hi:[1,0]" % (a(i), T(i), X) for i in range(np_)]
        if energy:
            L.append("v_add_f32 %%[en], %%[en], %s" % SQL)
        if np_ == 1:
            L.append("s_nop 0")
        L += ["v_pk_fma_f32 %s, %s, %s, %s neg_lo:[0,0,1] neg_hi:[0,0,1]" % (T(i), f(i), a(i), b(i)) for i in range(np_)]
        if np_ == 1:
            L.append("s_nop 0")
        L += ["v_pk_add_f32 %s, %s, %s op_sel:[0,1] op_sel_hi:[1,1]" % (b(i), T(i), X) for i in range(np_)]
        if energy:
            L.append("v_add_f32 %%[en], %%[en], %s" % SQH)
        return
    muls = ["v_pk_mul_f32 %s, %s, %s" % (T(i), f(i), b(i)) for i in range(np_)]
    if energy:
        # cvt, cvt, two products, the squares, the other products, first energy add
        head = muls[:2] + ["v_pk_mul_f32 %s, %s, %s" % (SQ, X, X)] + muls[2:]
        if np_ <= 2:
            head = muls + ["v_pk_mul_f32 %s, %s, %s" % (SQ, X, X)]
        L += head
        subs = ["v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (T(i), T(i), a(i)) for i in range(np_)]
        if np_ <= 2:
            # SQ was the last thing written: one subtraction in between
            L.append(subs[0])
            L.append("v_add_f32 %%[en], %%[en], %s" % SQL)
            L += subs[1:]
        else:
            L.append("v_add_f32 %%[en], %%[en], %s" % SQL)
            L += subs
    else:
        L += muls
        L += ["v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (T(i), T(i), a(i)) for i in range(np_)]
    if np_ == 1:
        L.append("s_nop 0")
    L += ["v_pk_add_f32 %s, %s, %s op_sel_hi:[1,0]" % (a(i), T(i), X) for i in range(np_)]
    if np_ == 1:
        L.append("s_nop 0")
    L += ["v_pk_mul_f32 %s, %s, %s" % (T(i), f(i), a(i)) for i in range(np_)]
    if np_ == 1:
        L.append("s_nop 0")
    L += ["v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (T(i), T(i), b(i)) for i in range(np_)]
    if np_ == 1:
        L.append("s_nop 0")
    L += ["v_pk_add_f32 %s, %s, %s op_sel:[0,1] op_sel_hi:[1,1]" % (b(i), T(i), X) for i in range(np_)]
    if energy:
        L.append("v_add_f32 %%[en], %%[en], %s" % SQH)


def body(np_, energy, fma=False):
    L = []
    L.append("s_waitcnt lgkmcnt(0)")                  # scalar loads of the compiler's may be out: they return out of order
    # entry: k0 == 0 first (every segment's first part), then a binary search
    L.append("s_cmp_eq_u32 %[k0], 0")
    L.append("s_cbranch_scc1 Le%=_0")

    def tree(lo, hi):
        if lo == hi:
            L.append("s_branch Le%%=_%d" % lo)
            return
        mid = (lo + hi + 1)//2
        L.append("s_cmp_lt_u32 %%[k0], %d" % mid)
        L.append("s_cbranch_scc1 Lt%%=_%d_%d" % (lo, mid - 1))
        tree(mid, hi)
        L.append("Lt%%=_%d_%d:" % (lo, mid - 1))
        tree(lo, mid - 1)
    tree(1, 15)
    # trampolines 1..15, then 0 falling into pair 0
    for k in list(range(1, 16)) + [0]:
        L.append("Le%%=_%d:" % k)
        for j in range(k, min(k + 3, 16)):
            L.append(read(j))
        if k != 0:
            L.append("s_branch Lp%%=_%d" % k)
    for k in range(16):
        L.append("Lp%%=_%d:" % k)
        if k + 3 < 16:
            L.append(read(k + 3))
        L.append("s_waitcnt lgkmcnt(%d)" % min(3, 15 - k))
        pair_block(L, np_, energy, fma, D(k))
        if k < 15:
            L.append("s_cmp_eq_u32 %%[k1], %d" % (k + 1))
            L.append("s_cbranch_scc1 Lx%=")
    L.append("Lx%=:")
    L.append("s_waitcnt lgkmcnt(0)")                  # reads past the exit land in the clobbered registers: before they are anybody else's
    return L


def common_parts(np_, energy, fma=False):
    """The common segment in the parts it is put together from: all sixteen pairs, chunk j (pairs 4j .. 4j+3) read whole from
    %[adj] into v[112+4j:115+4j].  Returns (reads, lead_in, pairs): the four reads; lead_in[k], what the body has done for pair k
    by the time it reaches it (its chunk waited for, its samples converted and squared); pairs[k], the pair itself.

    With no way in or out between the pairs, the work of a pair that is not the recurrence is spread one instruction at a time
    over the joints between the recurrence's groups (each group's first instruction waits for the first of the group before:
    that is where a lone wave has an issue slot to spare, and one only), and the converts and the squares run a pair ahead:
        muls f*b | energy += sq.lo | subs | cvt lo of the next pair | adds (+ x.lo) | energy += sq.hi |
        muls f*a | cvt hi of the next pair | subs | sq = squares of the next pair | adds (+ x.hi)
    The samples of an even pair are in X, those of an odd pair k in v(112+k-1) and v(112+k): the dwords of pairs k-1 and k, dead
    by the time pair k is converted (the high half in place)."""
    a = lambda i: "%%[a%d]" % i
    b = lambda i: "%%[b%d]" % i
    f = lambda i: "%%[f%d]" % i

    def xr(k):
        return (XL, XH) if k % 2 == 0 else ("v%d" % (112 + k - 1), "v%d" % (112 + k))

    def xp(k):
        return X if k % 2 == 0 else "v[%d:%d]" % (112 + k - 1, 112 + k)

    def cvt(k, half):
        return ("v_cvt_f32_i32_sdwa %s, sext(v%d) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_%d" % (xr(k)[half], 112 + k, half))

    def wait(k):
        # before pair k's first convert, if it opens a chunk (LDS reads return in order)
        return ["s_waitcnt lgkmcnt(%d)" % (3 - k//4)] if k % 4 == 0 else []

    def lead_in(k):
        out = ["s_waitcnt lgkmcnt(%d)" % (3 - k//4), cvt(k, 0), cvt(k, 1)]
        if energy:
            out.append("v_pk_mul_f32 %s, %s, %s" % (SQ, xp(k), xp(k)))
        return out

    reads = ["s_waitcnt lgkmcnt(0)"]                  # as above: from here on the counter counts the four reads alone
    for j in range(4):
        reads.append("ds_read_b128 v[%d:%d], %%[ad%d]" % (112 + 4*j, 115 + 4*j, j))
    pairs = []
    for k in range(16):
        L = []
        x = xp(k)
        nxt = k + 1 < 16
        add_lo = ["v_add_f32 %%[en], %%[en], %s" % SQL] if energy else []
        add_hi = ["v_add_f32 %%[en], %%[en], %s" % SQH] if energy else []
        cvt_lo = (wait(k + 1) + [cvt(k + 1, 0)]) if nxt else []
        cvt_hi = [cvt(k + 1, 1)] if nxt else []
        square = ["v_pk_mul_f32 %s, %s, %s" % (SQ, xp(k + 1), xp(k + 1))] if (nxt and energy) else []
        if fma:
            L += ["v_pk_fma_f32 %s, %s, %s, %s neg_lo:[0,0,1] neg_hi:[0,0,1]" % (T(i), f(i), b(i), a(i)) for i in range(np_)]
            L += add_lo
            L += ["v_pk_add_f32 %s, %s, %s op_sel_hi:[1,0]" % (a(i), T(i), x) for i in range(np_)]
            L += cvt_lo + cvt_hi
            L += ["v_pk_fma_f32 %s, %s, %s, %s neg_lo:[0,0,1] neg_hi:[0,0,1]" % (T(i), f(i), a(i), b(i)) for i in range(np_)]
            L += add_hi
            L += ["v_pk_add_f32 %s, %s, %s op_sel:[0,1] op_sel_hi:[1,1]" % (b(i), T(i), x) for i in range(np_)]
            L += square
        else:
            L += ["v_pk_mul_f32 %s, %s, %s" % (T(i), f(i), b(i)) for i in range(np_)]
            L += add_lo
            L += ["v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (T(i), T(i), a(i)) for i in range(np_)]
            L += cvt_lo
            L += ["v_pk_add_f32 %s, %s, %s op_sel_hi:[1,0]" % (a(i), T(i), x) for i in range(np_)]
            L += add_hi
            L += ["v_pk_mul_f32 %s, %s, %s" % (T(i), f(i), a(i)) for i in range(np_)]
            L += cvt_hi
            L += ["v_pk_add_f32 %s, %s, %s neg_lo:[0,1] neg_hi:[0,1]" % (T(i), T(i), b(i)) for i in range(np_)]
            L += square
            L += ["v_pk_add_f32 %s, %s, %s op_sel:[0,1] op_sel_hi:[1,1]" % (b(i), T(i), x) for i in range(np_)]
        pairs.append(L)
    return reads, [lead_in(k) for k in range(16)], pairs


def common_body(np_, energy, fma=False):
    reads, lead_in, pairs = common_parts(np_, energy, fma)
    return reads + lead_in[0] + [l for p in pairs for l in p]


def entry_tree():
    """k0 in 0 .. 15 to the leaf of its pair (tail bodies)."""
    L = []

    def tree(lo, hi):
        if lo == hi:
            L.append("s_branch Le%%=_%d" % lo)
            return
        mid = (lo + hi + 1)//2
        L.append("s_cmp_lt_u32 %%[k0], %d" % mid)
        L.append("s_cbranch_scc1 Lt%%=_%d_%d" % (lo, mid - 1))
        tree(mid, hi)
        L.append("Lt%%=_%d_%d:" % (lo, mid - 1))
        tree(lo, mid - 1)
    tree(0, 15)
    return L


def define(out, name, lines):
    out.append("#define %s \\" % name)
    for i, l in enumerate(lines):
        out.append('    "%s\\n\\t"%s' % (l, " \\" if i + 1 < len(lines) else ""))


def write_split(out):
    """The common segment once more, pair by pair (SPG_PC_*), and put together three ways: whole (what SPG_PAIRS_COMMON_ASM_* is),
    and as the two halves of the piece that holds a block end.  SPG_PAIRS_HEAD_ASM_* is pairs [0, k1): an exit test behind every
    pair -- what is converted and squared a pair ahead by then lies in clobbered registers and is dropped.  SPG_PAIRS_TAIL_ASM_*
    is pairs [k0, 16): the four reads, on their way while the entry tree is walked, a leaf per pair that does the pair's lead-in
    and joins the body at it, and no exit test anywhere."""
    define(out, "SPG_PC_READS", common_parts(2, 1)[0])
    define(out, "SPG_PC_TREE", entry_tree())
    for energy in (0, 1):
        lead = common_parts(2, energy)[1]
        for k in range(16):
            define(out, "SPG_PC_E%d_IN%d" % (energy, k), lead[k])
    for np_ in (2, 3, 4):
        for energy in (0, 1):
            pairs = common_parts(np_, energy)[2]
            for k in range(16):
                define(out, "SPG_PC_NP%d_E%d_P%d" % (np_, energy, k), pairs[k])
    out.append("#define SPG_PC_P(n, e, k) SPG_PC_NP##n##_E##e##_P##k")
    out.append('#define SPG_PC_OUT(k) "s_cmp_eq_u32 %[k1], " #k "\\n\\ts_cbranch_scc1 Lx%=\\n\\t"')
    out.append('#define SPG_PC_LEAF(e, k) "Le%=_" #k ":\\n\\t" SPG_PC_E##e##_IN##k "s_branch Lp%=_" #k "\\n\\t"')
    out.append('#define SPG_PC_AT(n, e, k) "Lp%=_" #k ":\\n\\t" SPG_PC_P(n, e, k)')
    out.append("#define SPG_PC_HEAD(n, e) SPG_PC_READS SPG_PC_E##e##_IN0 \\")
    out.append("    " + " ".join("SPG_PC_P(n, e, %d) SPG_PC_OUT(%d)" % (k, k + 1) for k in range(15)) + " \\")
    out.append('    SPG_PC_P(n, e, 15) "Lx%=:\\n\\ts_waitcnt lgkmcnt(0)\\n\\t"')
    out.append("#define SPG_PC_TAIL(n, e) SPG_PC_READS SPG_PC_TREE \\")
    out.append("    " + " ".join("SPG_PC_LEAF(e, %d)" % k for k in range(15, 0, -1)) + ' "Le%=_0:\\n\\t" SPG_PC_E##e##_IN0 \\')
    out.append("    " + " ".join("SPG_PC_AT(n, e, %d)" % k for k in range(16)))
    out.append("#define SPG_PC_WHOLE(n, e) SPG_PC_READS SPG_PC_E##e##_IN0 " + " ".join("SPG_PC_P(n, e, %d)" % k for k in range(16)))
    for np_ in (2, 3, 4):
        for energy in (0, 1):
            out.append("#define SPG_PAIRS_COMMON_ASM_NP%d_E%d SPG_PC_WHOLE(%d, %d)" % (np_, energy, np_, energy))
            out.append("#define SPG_PAIRS_HEAD_ASM_NP%d_E%d SPG_PC_HEAD(%d, %d)" % (np_, energy, np_, energy))
            out.append("#define SPG_PAIRS_TAIL_ASM_NP%d_E%d SPG_PC_TAIL(%d, %d)" % (np_, energy, np_, energy))
    out.append('#define SPG_PAIRS_SPLIT_ASM_CLOBBERS "memory", "scc", ' + ", ".join('"v%d"' % r for r in range(100, 128)))


def write(path, fma):
    out = []
    out.append("// %s -- GENERATED by tools/gen_pairs_asm.py; do not edit.  See that file and tone_fast.hpp (pairs_asm, pairs_common_asm, pairs_head_asm, pairs_tail_asm)." % os.path.basename(path))
    if fma:
        out.append("// The v_pk_fma_f32 form of the recurrence (fac*v2 - v1 fused: NOT the reference's roundings): only built with -DSPG_TONE_FMA.")
    for np_ in (2, 3, 4):
        for energy in (0, 1):
            define(out, "SPG_PAIRS_ASM_NP%d_E%d" % (np_, energy), body(np_, energy, fma))
    if fma:
        # (the experiment keeps the split bodies it was measured with: tone_fast.hpp builds no head and tail under SPG_TONE_FMA)
        for np_ in (2, 3, 4):
            for energy in (0, 1):
                define(out, "SPG_PAIRS_COMMON_ASM_NP%d_E%d" % (np_, energy), common_body(np_, energy, fma))
    else:
        write_split(out)
    out.append('#define SPG_PAIRS_ASM_CLOBBERS "memory", "scc", ' + ", ".join('"v%d"' % r for r in range(100, 116)))
    out.append('#define SPG_PAIRS_COMMON_ASM_CLOBBERS "memory", ' + ", ".join('"v%d"' % r for r in range(100, 128)))
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("wrote", os.path.normpath(path), len(out), "lines")


def main():
    write(OUT, False)
    write(OUT.replace("tone_pairs_asm.inc", "tone_pairs_asm_fma.inc"), True)


if __name__ == "__main__":
    main()
