#!/usr/bin/env python3
"""Two device-only compiles of gmr_amd/csrc/api.hip side by side: what a change to ik_body did to the ISA, read before any GPU run.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Wno-unused-value -S --cuda-device-only -o before.s gmr_amd/csrc/api.hip
    (the same for the changed tree, built at the same path)
    python tools/isa_stage_compare.py before.s after.s [--check]

It answers four questions ("Shared stage tables"); with --check it exits 1 if one of them has the wrong answer:

1. Which kernels changed?  Every kernel outside `--changed` (default: the shaped instances, a name with "IkShape" in it) must have
   the same assembly text, line for line, up to the path-derived __hip_cuid symbol.
2. Registers of the changed kernels, from the code object metadata: no scratch, no spilled VGPR, at most 256 VGPRs (two wavefronts per
   SIMD).  VGPRs, SGPR spills and static instruction counts are printed before and after.
3. The floating-point skeleton.  The loop nest of a shaped instance is read from the compiler's own loop comments: the frame loop is
   the depth-1 loop with the most instructions, the stage loop its largest child, the solve loop the stage loop's largest child.  The
   ordered sequence of float64 opcodes (every mnemonic with _f64 in it: fma / fmac / mul / add / max / min and their DPP forms, rcp,
   rsq, conversions, compares; operands stripped) of the solve loop, and of the frame loop outside the solve loop (the stage-entry
   residual; the compiler is free to peel the first stage's entry out of the stage loop, so the two are taken together), must be the
   same in both builds.  A re-contraction (a product and a sum becoming one fma, or the reverse) changes the opcodes and their counts
   and moves the bits.  The machine scheduler orders independent instructions of a block by register pressure, which changes the
   order alone: the report says which of the two it found, and --check fails on either.
   With --arith the multiset test is made on the ARITHMETIC float64 opcodes alone -- everything but the compares (v_cmp* / v_cmpx*),
   whose result is a lane mask, not a number -- over the frame loop as a whole (solve loop + the rest: which of the two the compiler
   lays a rotated loop's closing residual out with is its choice, and differs between toolchain layouts of the same code), and --check
   then fails on a different multiset only; the compares that differ are listed.  For a change that turns branches on a float64
   predicate into selects on the same predicate: the compare's encoding and sense change, no value does.
4. Vector memory reads inside the frame loop: global_load instructions in the stage loop (want: none after) and in the rest of the
   frame loop (the target block: unchanged).
"""
import argparse
import collections
import difflib
import re
import sys

FUNC = re.compile(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", re.S | re.M)
BLOCK = re.compile(r"^(?:\.LBB(\d+_\d+):|; %bb\.(\d+):)")
INSTR = re.compile(r"^\t([a-z]\w*)")


def functions(path):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(path).read())
    return {m.group(1): m.group(2) for m in FUNC.finditer(text)}, text


def metadata(text):
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        md = m.group(0)
        g = lambda k: int(re.search(k + r":\s+(\d+)", md).group(1))  # noqa: E731
        out[re.search(r"\.name:\s+(\S+)", md).group(1)] = dict(
            vgpr=g(r"\.vgpr_count"), agpr=g(r"\.agpr_count"), vspill=g(r"\.vgpr_spill_count"), sspill=g(r"\.sgpr_spill_count"),
            scratch=g(r"\.private_segment_fixed_size"), lds=g(r"\.group_segment_fixed_size"))
    return out


def blocks(body):
    """[(loop path, [mnemonics])] per basic block, in layout order.  The loop path of a block is the tuple of the headers of the loops
    around it, outermost first, from the "in Loop" / "Parent Loop" / "This Loop Header" comments."""
    out, path, ins, fn = [], (), [], None
    lines = body.split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        b = BLOCK.match(ln)
        if b:
            out.append((path, ins))
            ins = []
            name = b.group(1)
            if name:
                fn = name.split("_")[0]
            me = "BB" + name if name else None
            note = [ln]
            while i + 1 < len(lines) and re.match(r"^\s+;", lines[i + 1]):  # continuation lines of a header's comment
                i += 1
                note.append(lines[i])
            note = "\n".join(note)
            parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=\d+", note)
            inl = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            if "Loop Header: Depth=" in note:
                path = tuple(parents) + (me,)
            elif inl:
                path = ("?",) * (int(inl.group(2)) - 1) + (inl.group(1),)  # (outer headers unnamed here: resolved below)
            else:
                path = ()
        else:
            m = INSTR.match(ln)
            if m and not m.group(1).startswith("s_nop") and not ln.startswith("\t."):
                ins.append(m.group(1))
        i += 1
    out.append((path, ins))
    # resolve the unnamed outer headers: a loop header names all of its parents
    full = {p[-1]: p for p, _ in out if p and "?" not in p}
    return [((full.get(p[-1], p) if p else p), ins) for p, ins in out]


def largest_child(bl, prefix):
    size = {}
    for p, ins in bl:
        if len(p) > len(prefix) and p[:len(prefix)] == prefix:
            size[p[len(prefix)]] = size.get(p[len(prefix)], 0) + len(ins)
    return max(size, key=size.get) if size else None


def regions(body):
    """The mnemonics, in layout order, of: the frame loop outside the stage loop, the stage loop outside the solve loop, the solve loop."""
    bl = blocks(body)
    frame = largest_child(bl, ())
    stage = largest_child(bl, (frame,))
    solve = largest_child(bl, (frame, stage))
    pick = lambda pred: [op for p, ins in bl if pred(p) for op in ins]  # noqa: E731
    return dict(
        frame_rest=pick(lambda p: p[:1] == (frame,) and p[:2] != (frame, stage)),
        stage_entry=pick(lambda p: p[:2] == (frame, stage) and p[:3] != (frame, stage, solve)),
        solve=pick(lambda p: p[:3] == (frame, stage, solve)),
        whole=[op for _, ins in bl for op in ins])


def f64(ops):
    return [o for o in ops if "_f64" in o]


def is_cmp(op):
    return op.startswith("v_cmp")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--changed", default="IkShape", help="substring of the kernels that are allowed to differ")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--arith", action="store_true", help="test the arithmetic float64 opcodes (no compares) of the whole frame loop as a multiset")
    a = ap.parse_args()
    (fa, ta), (fb, tb) = functions(a.before), functions(a.after)
    ma, mb = metadata(ta), metadata(tb)
    bad = []

    print("## 1. kernels whose assembly differs")
    kernels = [k for k in fa if k in ma]
    if set(fa) != set(fb):
        bad.append("the two builds do not hold the same functions: %s" % sorted(set(fa) ^ set(fb)))
    differ = [k for k in fa if k in fb and fa[k] != fb[k]]
    for k in differ:
        ok = a.changed in k
        print("  %s %s" % ("changed " if ok else "CHANGED?", k))
        if not ok:
            bad.append("assembly of %s differs" % k)
    print("  %d kernels (%d functions), %d differ; every other one is identical line for line" % (len(kernels), len(fa), len(differ)))
    if {k: v for k, v in ma.items() if a.changed not in k} != {k: v for k, v in mb.items() if a.changed not in k}:
        bad.append("resource metadata of an unchanged kernel differs")

    print("\n## 2. registers of the changed kernels (before -> after)")
    print("  %-44s %11s %11s %9s %9s %13s %15s" % ("kernel", "vgpr", "sgpr spill", "vspill", "scratch", "instructions", "waves/SIMD"))
    reg = {}
    for k in sorted(k for k in fa if a.changed in k and k in ma and k in mb):
        short = re.sub(r"^_ZN3gmr\d+", "", k).split("EEEv")[0]
        x, y = ma[k], mb[k]
        ra, rb = regions(fa[k]), regions(fb[k])
        reg[k] = (ra, rb)
        occ = lambda r: min(8, 512 // max(-(-(r["vgpr"] + r["agpr"]) // 8) * 8, 8))  # noqa: E731
        print("  %-44s %4d -> %4d %4d -> %4d %3d -> %3d %3d -> %3d %5d -> %5d %6d -> %6d" % (
            short, x["vgpr"], y["vgpr"], x["sspill"], y["sspill"], x["vspill"], y["vspill"], x["scratch"], y["scratch"],
            len(ra["whole"]), len(rb["whole"]), occ(x), occ(y)))
        if y["vspill"] or y["scratch"] or y["vgpr"] + y["agpr"] > 256 or occ(y) < 2:
            bad.append("%s: scratch, spilled VGPRs or more than 256 registers" % short)

    print("\n## 3. float64 opcode sequences (operands stripped), and 4. global_load in the frame loop")
    for k, (ra, rb) in reg.items():
        short = re.sub(r"^_ZN3gmr\d+", "", k).split("EEEv")[0]
        print("  " + short)
        for r in (ra, rb):  # (where the first stage's residual sits -- in the stage loop or peeled in front of it -- is the compiler's choice)
            r["outside_solve"] = r["frame_rest"] + r["stage_entry"]
        for name in ("solve", "outside_solve", "whole"):
            sa, sb = f64(ra[name]), f64(rb[name])
            same, same_set = sa == sb, sorted(sa) == sorted(sb)
            moved = sum(j2 - j1 for tag, _, _, j1, j2 in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes() if tag in ("insert", "replace"))
            print("    %-13s instructions %5d -> %5d   float64 opcodes %4d -> %4d  %s" % (
                name, len(ra[name]), len(rb[name]), len(sa), len(sb),
                "equal in order" if same else "ORDER DIFFERS (%d opcodes sit elsewhere); as multisets %s" % (moved, "equal" if same_set else "DIFFERENT")))
            if not same_set:
                ca, cb = collections.Counter(sa), collections.Counter(sb)
                print("      gone: %s   new: %s" % (dict(ca - cb), dict(cb - ca)))
            if not same and name != "whole" and not a.arith:
                bad.append("%s: float64 opcode sequence of %s differs%s" % (short, name, " in order only (same opcodes, same counts)" if same_set else ""))
        if a.arith:
            fa_, fb_ = f64(ra["solve"] + ra["outside_solve"]), f64(rb["solve"] + rb["outside_solve"])
            aa, ab_ = collections.Counter(o for o in fa_ if not is_cmp(o)), collections.Counter(o for o in fb_ if not is_cmp(o))
            ca, cb = collections.Counter(o for o in fa_ if is_cmp(o)), collections.Counter(o for o in fb_ if is_cmp(o))
            print("    frame loop    arithmetic float64 opcodes %4d -> %4d  as multisets %s;  float64 compares %d -> %d%s" % (
                sum(aa.values()), sum(ab_.values()), "equal" if aa == ab_ else "DIFFERENT", sum(ca.values()), sum(cb.values()),
                "" if ca == cb else "  gone: %s   new: %s" % (dict(ca - cb), dict(cb - ca))))
            if aa != ab_:
                print("      gone: %s   new: %s" % (dict(aa - ab_), dict(ab_ - aa)))
                bad.append("%s: arithmetic float64 opcodes of the frame loop differ as multisets" % short)
        gl = lambda ops: sum(o.startswith("global_load") for o in ops)  # noqa: E731
        ga, gb = [gl(ra[n]) for n in ("frame_rest", "stage_entry", "solve")], [gl(rb[n]) for n in ("frame_rest", "stage_entry", "solve")]
        print("    global_load  target block / rest of frame %d -> %d, stage entry %d -> %d, solve loop %d -> %d" % (
            ga[0], gb[0], ga[1], gb[1], ga[2], gb[2]))
        if gb[1] or gb[2] or gb[0] > ga[0]:
            bad.append("%s: a global_load is left in the stage loop, or the target block gained one" % short)
        ds = lambda ops: sum(o.startswith("ds_read") or o.startswith("ds_load") for o in ops)  # noqa: E731
        print("    LDS reads    stage entry %d -> %d, solve loop %d -> %d" % (ds(ra["stage_entry"]), ds(rb["stage_entry"]), ds(ra["solve"]), ds(rb["solve"])))

    print("\n" + ("FAILED:\n  " + "\n  ".join(bad) if bad else "all four hold"))
    if a.check and bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
