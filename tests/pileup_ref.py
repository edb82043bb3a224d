"""The contract of `align_pileup` (include/rattle_hip.h) in plain Python: the table kernel G fills, from the records and the CIGAR strings
of a case alone.  Written from the header's table, not from the kernel.

One table over the concatenated targets, N = sum of their lengths positions, eight counts per position (FIELDS), all on the TARGET's
strand.  For every read with status 0 whose rectangle has a column (t_end > t_start), walk its CIGAR as `align_cigars` defines it -- the
read reverse-complemented first when rev == 1, the target forward, U read as T -- from t_start, j the target position, i the row of the
aligned read:

  a, c, g, t at j   a column of an '=' or 'X' op whose read base (on the aligned strand) is that letter
  del at j          a column of a 'D' op
  ins at j          an 'I' op that is neither the first nor the last op of the CIGAR, once per op, at the position of the column that
                    follows it
  starts at t_start, ends at t_end - 1     once per such read

A leading or trailing I run (read mode: the read's overhang), a read-mode pair with t_end == t_start and a read whose status is not 0 add
nothing.  depth = a + c + g + t + del.

  table(targets, reads, target_of_read, rev, records, cigar_texts)   the eight lists, in FIELDS order
  identities(table, records)                                         the four sums the header promises, as a list of what fails
  model(case, sc, mode)                                              (records, CIGAR strings, table) of a case from tests/align_model.py

and the cases aimed at kernel G's own edges: rounds of 64 ops, column steps of 64, many reads on few positions, neighbouring targets;
ins_pairs(), one interior I op at a chosen op index -- 1, 63, 64, 65, 127, 128, the last but one, with the op count on a round's edge,
beside a read-mode overhang that is alone in its round or is op 0 -- each with the position it counts at; reverse_given(), a read as it
is handed over on the other strand; gap_contention_case(), 4096 reads with a D run and an I run on the same positions.
No device, no numpy in the walk."""
import re

import numpy as np

import align_affine_ref as AF
import align_model as M
import align_ref as R

FIELDS = ("a", "c", "g", "t", "del", "ins", "starts", "ends")
A_, C_, G_, T_, DEL, INS, STARTS, ENDS = range(8)
_LETTER = {ord("A"): A_, ord("C"): C_, ord("G"): G_, ord("T"): T_}
_OP = re.compile(rb"(\d+)([=XID])")
LINEAR, ENGINE, MM2 = AF.LINEAR, AF.ENGINE, AF.MM2
FORMS = tuple((sc, mode) for sc in (LINEAR, ENGINE, MM2) for mode in M.MODES)


def parse(text: bytes):
    """b"3I10=2I5=4I" -> [(b"I", 3), (b"=", 10), ...]; every byte of the string has to belong to an op"""
    ops = [(o, int(n)) for n, o in _OP.findall(text)]
    assert b"".join(b"%d%s" % (n, o) for o, n in ops) == text, text
    return ops


def table(targets, reads, target_of_read, rev, records, cigar_texts):
    base = [0]
    for t in targets:
        base.append(base[-1] + len(t))
    planes = [[0] * base[-1] for _ in FIELDS]
    for r, (q, x, s) in enumerate(zip(reads, target_of_read, rev)):
        if int(records["status"][r]) != 0:
            continue
        ts, te = int(records["t_start"][r]), int(records["t_end"][r])
        if te <= ts:
            continue
        qs, qe = int(records["q_start"][r]), int(records["q_end"][r])
        aligned = (R.revcomp(q) if int(s) else q).translate(R._T)
        i = len(q) - qe if int(s) else qs                      # the record is on the read as given
        j = base[x] + ts
        planes[STARTS][j] += 1
        planes[ENDS][base[x] + te - 1] += 1
        ops = parse(cigar_texts[r])
        for k, (o, n) in enumerate(ops):
            if o in (b"=", b"X"):
                for _ in range(n):
                    planes[_LETTER[aligned[i]]][j] += 1
                    i += 1
                    j += 1
            elif o == b"D":
                for _ in range(n):
                    planes[DEL][j] += 1
                    j += 1
            else:
                if 0 < k < len(ops) - 1:
                    planes[INS][j] += 1
                i += n
        assert j == base[x] + te and i == (len(q) - qs if int(s) else qe), (r, cigar_texts[r])
    return planes


def as_lists(pileup: dict):
    """what Context.align_pileup returned, as table() returns it"""
    return [[int(v) for v in pileup[f]] for f in FIELDS]


def depth(planes):
    return [sum(v) for v in zip(*planes[:DEL + 1])]


def identities(planes, records):
    """the header's four sums; returns the names of those that fail"""
    ok = np.asarray(records["status"]) == 0
    col = ok & (np.asarray(records["t_end"]) > np.asarray(records["t_start"]))
    bad = []
    if sum(sum(p) for p in planes[:4]) != int(np.asarray(records["matches"])[ok].sum()) + int(np.asarray(records["mismatches"])[ok].sum()):
        bad.append("letters")
    if sum(planes[DEL]) != int(np.asarray(records["t_gap"])[ok].sum()):
        bad.append("del")
    if sum(planes[STARTS]) != int(col.sum()) or sum(planes[ENDS]) != int(col.sum()):
        bad.append("starts/ends")
    if any(n and not d for n, d in zip(planes[INS], depth(planes))):
        bad.append("ins without depth")
    return bad


_memo = {}


def model(name, case, sc, mode, max_cells=0):
    """(records, CIGAR strings, table) of the case under tests/align_model.py; remembered under `name`, and handed out to be left alone"""
    key = (name, tuple(sc), mode, max_cells)
    if key not in _memo:
        rec = M.records(*case, sc, mode, max_cells)
        cg = M.cigars(*case, sc, mode, max_cells)
        _memo[key] = (rec, cg, table(*case, rec, cg))
    return _memo[key]


# ---- cases for kernel G: (targets, reads, target_of_read, rev) ----------------------------------------------------------------------
def _other(c: int, k: int = 1) -> int:
    return b"ACGT"[(b"ACGT".index(c) + k) % 4]


def thirds_pair(L: int, seed: int, extra=None):
    """(read, target): a random target of L bases and the read equal to it with every third base (indices 2, 5, ...) substituted: the
    CIGAR is 2=1X2=1X...  extra = k: the read also lacks base k + 1 of the target (k a substituted index), so an X run and a D run
    stand side by side and the number of ops is even where it was odd."""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, L)
    q = bytearray(_other(c) if i % 3 == 2 else c for i, c in enumerate(t))
    if extra is not None:
        del q[extra + 1]
    return bytes(q), t


# name -> (scoring, mode, ops the model has to give, read, target): the pairs whose op count sits on a round of 64 ops
def op_count_pairs():
    out = {}
    for sc, mode, L, ops in ((LINEAR, M.LOCAL, 94, 63), (LINEAR, M.LOCAL, 97, 65), (LINEAR, M.LOCAL, 191, 127), (LINEAR, M.LOCAL, 193, 129),
                             (ENGINE, M.READ, 96, 64), (ENGINE, M.READ, 192, 128)):
        out["%s_%d" % (mode, ops)] = (sc, mode, ops) + thirds_pair(L, 200 + L)
    # locally a final X is clipped, so an even count takes a gap beside an X (thirds_pair's `extra`); the assertion decides
    out["local_64"] = (LINEAR, M.LOCAL, 64) + thirds_pair(95, 195, extra=47)
    out["local_128"] = (LINEAR, M.LOCAL, 128) + thirds_pair(191, 291, extra=95)
    return out


def n_ops(q, t, sc, mode):
    return len(M.pair(q, t, 0, sc, mode)[1])


def ins_pair(L: int, at: int, base: bytes, extra=None, lead=b"", trail=b"", seed=7):
    """(read, target): thirds_pair(L, seed, extra) with `base` put into the read in front of its base `at` -- one I op between the
    2= and 1X runs, at about op 2 at / 3 -- and with `lead` in front of the read and `trail` behind it (read mode: the overhangs)"""
    q, t = thirds_pair(L, seed, extra)
    return lead + q[:at] + base + q[at:] + trail, t


# name -> (arguments of ins_pair, {mode: (ops, index of the one interior I op, target position that op counts at)}).  A round of kernel
# G takes 64 ops, so index 63 is the last lane of round 0, 64 the first of round 1, 127 and 128 the same one round on; `ops - 2` is the
# last op that can count.  `extra` shifts the parity of the later indices: without it every I op of these pairs has an odd index.
# The numbers are what tests/align_model.py gives, found once by a search over `at`, `base` and `extra`; ins_pairs() asserts them.
INS_PAIRS = {
    "index_1": ((200, 2, b"G"), {M.LOCAL: (133, 1, 3), M.READ: (133, 1, 3)}),
    "index_63": ((200, 95, b"G"), {M.LOCAL: (133, 63, 96), M.READ: (133, 63, 96)}),
    "index_63_of_65": ((98, 95, b"G"), {M.LOCAL: (65, 63, 96), M.READ: (65, 63, 96)}),           # the one op behind it is in round 1
    "index_64": ((200, 94, b"G", 20), {M.LOCAL: (134, 64, 96), M.READ: (134, 64, 96)}),
    "index_64_of_66": ((98, 94, b"G", 20), {M.LOCAL: (66, 64, 96), M.READ: (66, 64, 96)}),       # lane 0 of round 1, one op behind it
    "index_65": ((200, 94, b"G", 50), {M.LOCAL: (135, 65, 96), M.READ: (135, 65, 96)}),
    "index_127": ((200, 191, b"T"), {M.LOCAL: (133, 127, 192), M.READ: (133, 127, 192)}),
    "index_127_of_129": ((193, 191, b"T"), {M.READ: (129, 127, 192)}),
    "index_128": ((200, 190, b"T", 20), {M.LOCAL: (134, 128, 192), M.READ: (134, 128, 192)}),
    "index_131_of_133": ((200, 197, b"A"), {M.LOCAL: (133, 131, 198), M.READ: (133, 131, 198)}),
    # read mode: an overhang that is op 64 of 65, alone in round 1, and one that is op 0 of 134; neither counts, the I inside does
    "trailing_overhang": ((95, 50, b"G", None, b"", b"GTTGTTT"), {M.READ: (65, 33, 50)}),
    "leading_overhang": ((200, 95, b"G", None, b"CTT"), {M.READ: (134, 64, 96)}),
}
INS_SCORING = {M.LOCAL: LINEAR, M.READ: ENGINE}


def interior_ins(ops):
    """[(index, target columns in front of it)] of the I ops that are neither the first nor the last op"""
    out, cols = [], 0
    for k, (o, n) in enumerate(ops):
        if o == "I" and 0 < k < len(ops) - 1:
            out.append((k, cols))
        if o != "I":
            cols += n
    return out


INS_FORMS = tuple((name, mode) for name, (_, forms) in INS_PAIRS.items() for mode in forms)


def ins_pairs(name, mode):
    """(scoring, ops, index, position, read, target) of INS_PAIRS[name] under `mode`, asserted through the model: that many ops, one
    interior I op, at that index, counted at that target position; the overhang pairs begin or end with an I op, no other does"""
    args, forms = INS_PAIRS[name]
    ops, index, position = forms[mode]
    q, t = ins_pair(*args)
    rec, got = M.pair(q, t, 0, INS_SCORING[mode], mode)
    assert len(got) == ops and interior_ins(got) == [(index, position - rec[4])], (name, mode, len(got), interior_ins(got), rec[4])
    assert (got[0][0] == "I") == (name == "leading_overhang") and (got[-1][0] == "I") == (name == "trailing_overhang"), name
    return INS_SCORING[mode], ops, index, position, q, t


def reverse_given(q: bytes) -> bytes:
    """the read as it is handed over for rev = 1: reverse-complemented and written with U"""
    return R.revcomp(q).replace(b"T", b"U")


GAP_COPIES = 4096


def gap_contention_pair(seed=58):
    """(read, target): a target of 101 bases and the 100-base read that lacks its bases 35 .. 37 and holds two more in front of its
    base 70; under 5,4,8,6 the flanks of 35, 32 and 31 carry both gaps: 35=3D32=2I31= (asserted where it is used)"""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 101)
    extra = bytes([_other(t[70]), _other(t[70], 2)])
    return t[:35] + t[38:70] + extra + t[70:], t


GAP_CONTENTION_CIGAR = b"35=3D32=2I31="


def gap_contention_case(seed=58):
    """4096 copies of gap_contention_pair's read on its target, every second one handed over on the other strand"""
    q, t = gap_contention_pair(seed)
    back = reverse_given(q)
    n = GAP_COPIES
    return [t], [back if r % 2 else q for r in range(n)], [0] * n, [r % 2 for r in range(n)]


def identical_case(seed=51):
    """identical pairs of 1, 63, 64, 65 and 129 bases: one '=' run, across a column step of 64 from 65 on; the first is the pair of
    one column"""
    rng = np.random.default_rng(seed)
    return R.pairs_case([(s, s, 0) for s in (R.rnd(rng, n) for n in (1, 63, 64, 65, 129))])


def long_gap_case():
    """exon_pair with inserts of 63, 64 and 65 in the target (a D run across a column step) and the same with the insert in the read
    (an I run: rows that no column step sees); 120-base flanks, so that 5,4,8,6 spans the gap"""
    pairs = []
    for n in (63, 64, 65):
        q, t = AF.exon_pair(seed=60 + n, flank=120, insert=n)
        pairs += [(q, t, 0), (t, q, 0)]
    return R.pairs_case(pairs)


CONTENTION_COPIES = 4096


def contention_case(seed=52):
    """4096 copies of one 70-base read on one 70-base target, every second one handed over reverse-complemented (and written with U)"""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 70)
    back = R.revcomp(t).replace(b"T", b"U")
    n = CONTENTION_COPIES
    return [t], [back if r % 2 else t for r in range(n)], [0] * n, [r % 2 for r in range(n)]


def neighbours_case(seed=53):
    """Three targets of 80, 90 and 50 bases; reads that end on the last base of target 0 and begin on base 0 of target 1 (both strands),
    nothing on target 2; a read that is not submitted, an empty read, and a read that max_cells = NEIGHBOURS_MAX_CELLS leaves out."""
    rng = np.random.default_rng(seed)
    t0, t1, t2 = R.rnd(rng, 80), R.rnd(rng, 90), R.rnd(rng, 50)
    reads = [t0[30:], t1[:40], R.revcomp(t0[45:]), R.revcomp(t1[:33]), t0[10:60], b"", t1]
    return [t0, t1, t2], reads, [0, 1, 0, 1, -1, 1, 1], [0, 0, 1, 1, 0, 0, 0]


NEIGHBOURS_MAX_CELLS = 80 * 90 - 1           # read 6 (90 bases on the 90 of target 1) is over it, no other read is


def read_mode_case(seed=54):
    """read mode under 5,4,8,6: a leading overhang, a trailing one, both, each with an insertion of 6 bases in the middle of the read
    (the one I run that counts, at the base to its right); and CC on AA, which under 1,64,1,1 has no column"""
    rng = np.random.default_rng(seed)
    t = R.rnd(rng, 120)                          # the read covers the whole target: what overhangs has no target base to stand on
    mid = t[:60] + CG_INSERT + t[60:]
    return R.pairs_case([(R.rnd(rng, 9) + mid, t, 0), (mid + R.rnd(rng, 7), t, 0), (R.rnd(rng, 5) + mid + R.rnd(rng, 8), t, 0)])


CG_INSERT = b"GATTAC"


CASES = {"identical": identical_case, "long_gaps": long_gap_case, "neighbours": neighbours_case, "read_mode": read_mode_case}
