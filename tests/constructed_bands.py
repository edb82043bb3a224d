"""Packs built so that an alignment of kernel C's exact band (poa.hip step 3a, `dp_rows_band`) sits ON one of the comparisons
its plan is made of, and a model of that plan.  No GPU and no oracle in here: tests/test_constructed_bands.py proves through
Oracle.poa_band that every pack sits where it is named, and tests/test_gpu_poa_band_edges.py then runs the same packs through the kernel
and compares its counters with the model's, so a GPU case cannot go vacuous.

The model (`plan_pack`) is written from DESIGN.md §4 ("The band", "The certificate", "The plan of an alignment"), not from the kernel.  It
takes the facts of Oracle.poa_band -- per alignment the graph's rows n and MSA columns C, the read's length L, the best score S of the full
matrices, and whether the columns order the edges -- and returns per alignment the attempts (cplb, t, s, certified).  By the lemma an
attempt is certified iff S >= 5 (L - t) - 4: when the certificate passes, the band's best score IS S; when it fails the band's best score
is <= S and below the bound.  So S is all the model needs of the matrices.

The packs.  `base` is a fixed-seed random sequence; "junk" is a run that cannot extend the local alignment: every junk letter differs from
the base letters it faces on the main diagonal and on the two diagonals beside it (and never pays for a gap: 5 k < 8 for one base).  What a
case claims -- its S, the diagonal its optimal path runs on -- is in its dict, and the CPU test checks it against the oracle's numbers."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
ACG = np.frombuffer(b"ACG", np.uint8)
MATCH = 5
SUB_COST = 9                     # a substitution inside a matched run: a match lost (5) and a mismatch paid (4)
LADDER = (2, 4, 8)               # columns per lane, in the order the plan tries them
STRIP_COLS = 512
STRIPS_MIN_OK = 8


# ---- the plan, from DESIGN.md §4 ----
def width(C, L, cplb):
    """(t, s) of the window of 64 lanes x cplb columns for a read of L against C columns, or None where the plan skips that form: the
    window holds C - L + 2 t + 1 <= 63 cplb columns, t takes all that room but at most L - 1, and tau = L - t <= C"""
    room = 63 * cplb - 1 - (C - L)
    if room < 0:
        return None
    t = min(room >> 1, L - 1)
    if C < L - t:
        return None
    return t, C + t - L


def threshold(L, t):
    """the certificate's bound: a best score of at least this much cannot be reached through a cell outside the window"""
    return MATCH * (L - t) - 4


def plan_pack(facts, debug=0):
    """The plan of every alignment of one pack.  facts: Oracle.poa_band(pack).  debug: RATTLE_POA_DEBUG (8: strips for every alignment
    without a band, 16: no band attempts).  Returns a dict: alignments -- per alignment {"attempts": [(cplb, t, s, certified)], "how":
    "band" | "strips" | "back"} up to and including the one that hands the pack back; ok / fail -- certified alignments and failed
    certificates; strips -- alignments over the full rows as strips; cells -- what the band pass computes; back -- the alignment (1-based)
    at which the pack is handed back to the full-row kernels, or None."""
    out = {"alignments": [], "ok": 0, "fail": 0, "strips": 0, "cells": 0, "back": None}
    t_hist = 0
    for k, f in enumerate(facts, 1):
        n, C, L, S = f["n"], f["C"], f["L"], f["S"]
        attempts, certified, unordered = [], False, False
        t_want = max(8, 2 * t_hist + 4)
        for cplb in LADDER if not debug & 16 else ():
            w = width(C, L, cplb)
            if w is None or (cplb == 2 and w[0] < t_want):
                continue
            if not f["ordered"]:
                unordered = True                    # seen while the rows' records are built: no band, and no strips either
                break
            t, s = w
            certified = S >= threshold(L, t)
            attempts.append((cplb, t, s, certified))
            out["cells"] += n * 64 * cplb
            if certified:
                out["ok"] += 1
                t_hist = (MATCH * L - S) // MATCH
                break
            out["fail"] += 1
        how = "band"
        if not certified:
            earned = bool(debug & 8) or (out["ok"] >= STRIPS_MIN_OK and 4 * out["ok"] >= 3 * k)
            if earned and not unordered:
                how = "strips"
                out["strips"] += 1
                out["cells"] += n * STRIP_COLS * (-(-L // STRIP_COLS))
            else:
                how = "back"
        out["alignments"].append({"attempts": attempts, "how": how})
        if how == "back":
            out["back"] = k
            break
    return out


# ---- sequences ----
def backbone(seed, L, letters=ACGT):
    return letters[np.random.default_rng(seed).integers(0, len(letters), L)].copy()


def junk(base, lo, hi):
    """hi - lo letters for read positions lo .. hi-1: each differs from base[i - 1], base[i] and base[i + 1] (the letters it faces on the main
    diagonal and beside it; beyond the base's ends nothing is faced) and, where a letter is left for that, from base[i - 2] and base[i + 2]"""
    out = np.zeros(hi - lo, np.uint8)
    for i in range(lo, hi):
        faced = {int(base[j]) for j in (i - 1, i, i + 1) if 0 <= j < len(base)}
        free = [c for c in ACGT if int(c) not in faced]
        beside = {int(base[j]) for j in (i - 2, i + 2) if 0 <= j < len(base)}
        free = [c for c in free if int(c) not in beside] or free
        out[i - lo] = free[i % len(free)]
    return out


def substituted(seq, pos):
    out = seq.copy()
    out[pos] = ACGT[(int(np.nonzero(ACGT == seq[pos])[0][0]) + 1 + pos % 3) % 4]
    return out


def _b(*parts):
    return b"".join(np.asarray(p, np.uint8).tobytes() for p in parts)


# ---- the edge families: the third read of [base, base, read] ----
RIGHT_N = 460                     # the base of the right-edge and diagonal cases: C = L = 460, t = 62 / 125 / 251
LEFT_N, LEFT_D = 500, 40          # the base of the left-edge cases and the 5' cut: C - L = 40, t = 42 / 105 / 231
VARIANTS = ("on", "sub", "off")   # m = t; m = t - 1 and a substitution; m = t + 1


# (family, cplb) -> the base's seed, where the default one gave the junk a chance extension (test_constructed_bands.py caught it)
EDGE_SEEDS = {("diag", 4): 1000, ("diag", 8): 1000}


def _edge_case(family, cplb, variant, seed=None):
    """one case of a family at the width of `cplb` columns per lane.  m junk bases, the rest a run of the base on one diagonal:
    right -- junk(m) + base[:N - m]: read column j faces graph column j - m, the optimal path lies m columns RIGHT of the rows' columns;
    diag  -- junk(m) + base[m:]: the same score on the main diagonal (the certificate's edge alone, the path in mid-window);
    left  -- base[d + m:] + junk(m): the path lies d + m columns LEFT of the rows' columns (C - L = d)."""
    N, d = (LEFT_N, LEFT_D) if family == "left" else (RIGHT_N, 0)
    if seed is None:
        seed = EDGE_SEEDS.get((family, cplb), {"right": 11, "diag": 12, "left": 13}[family] * 10 + cplb)
    base = backbone(seed, N)
    L = N - d
    t, s = width(N, L, cplb)
    m = {"on": t, "sub": t - 1, "off": t + 1}[variant]
    if family == "right":
        run, offset = base[:N - m], m
        read = np.concatenate([junk(base, 0, m), run])
        sub_at = m + len(run) // 2
    elif family == "diag":
        run, offset = base[m:], 0
        read = np.concatenate([junk(base, 0, m), run])
        sub_at = m + len(run) // 2
    else:
        run, offset = base[d + m:], -(d + m)
        read = np.concatenate([run, junk(base, L - m, L)])
        sub_at = len(run) // 2
    S = MATCH * (L - m)
    if variant == "sub":
        read = substituted(read, sub_at)
        S -= SUB_COST
    assert len(read) == L
    return {"pack": [_b(base), _b(base), _b(read)], "family": family, "edge": 2, "cplb": cplb, "t": t, "s": s, "m": m, "S": S,
            "offset": offset, "certified_here": variant != "off", "base": _b(base)}


# ---- the clamp t = L - 1 ----
def _clamp_cases():
    """A short third read against a graph of 300 (or 320) columns of A / C / G; junk is T, which the graph does not hold: S is exact.  Only
    the 8-column form has room, and there t = L - 1, tau = 1: any match certifies, none does not.
    20 nt against 300 columns: the only form with room is the 8-column one, clamped.  62 / 63 nt against 300 columns: the 4-column form
    has room for t = 6 / 7 and certifies a read that matches throughout (named `wide`: not at the clamp); against 320 columns it has none
    and the clamp is reached.  63 nt of which 20 match, against 300 columns: fails at t = 7, certified at the clamp.  63 nt of junk: S = 0,
    fails at every width."""
    cases = {}
    for N in (300, 320):
        base = backbone(14 + N, N, ACG)
        for L in ((20, 62, 63) if N == 300 else (62, 63)):
            read = base[100:100 + L]
            name = "clamp_%d" % L if (N == 320 or L == 20) else "clamp_wide_%d" % L
            cases[name] = {"pack": [_b(base), _b(base), _b(read)], "family": "clamp", "edge": 2, "S": MATCH * L, "clamped": "wide" not in name}
    base = backbone(14 + 300, 300, ACG)
    T = np.full(63, ord("T"), np.uint8)
    cases["clamp_63_part"] = {"pack": [_b(base), _b(base), _b(base[100:120], T[:43])], "family": "clamp", "edge": 2, "S": 100, "clamped": True}
    cases["clamp_63_junk"] = {"pack": [_b(base), _b(base), _b(T)], "family": "clamp", "edge": 2, "S": 0, "clamped": True}
    return cases


# ---- the skip C < L - t ----
SKIP_N = 300


def skip_edge(cplb):
    """the largest 3' extension e of a read over a graph of SKIP_N columns at which the form of `cplb` columns is still tried (tau = L - t
    <= C); one more and it is skipped"""
    e = 0
    while width(SKIP_N, SKIP_N + e + 1, cplb) is not None:
        e += 1
    return e


def _skip_cases():
    base = backbone(15, SKIP_N)
    ext = backbone(16, 400)
    cases = {}
    for cplb in (2, 4):
        e0 = skip_edge(cplb)
        for e, tried in ((e0, True), (e0 + 1, False)):
            read = _b(base, ext[:e])
            cases["skip_%d_%s" % (cplb, "tried" if tried else "skipped")] = {
                "pack": [_b(base), read, read], "family": "skip", "edge": 1, "cplb": cplb, "e": e, "tried": tried, "S": MATCH * SKIP_N}
    return cases


# ---- the history rule ----
HIST_N = 400


def _history_cases():
    """[X[h:], X[h:], junk(h) + X[h:], junk(h) + X[h:]]: the second alignment is certified with a score 5 h below 5 L (t_hist = h) and
    gives the graph h columns in front; the third is clean with C = L, where the 2-column form has t = 62: tried after h = 29 (t_want 62),
    skipped after h = 30 (t_want 64)"""
    X = backbone(17, HIST_N)
    cases = {}
    for h in (29, 30):
        read = _b(junk(X, 0, h), X[h:])
        cases["history_%d" % h] = {"pack": [_b(X[h:]), _b(X[h:]), read, read], "family": "history", "h": h, "S": [MATCH * (HIST_N - h)] * 2 + [MATCH * HIST_N]}
    return cases


# ---- earned strips ----
STRIPS_N = 600


def _strips_cases():
    """clean reads (the base with one substitution each) and reads with 300 nt removed, which no window holds: the 9th alignment after 8
    certified ones has earned the strips, the 8th after 7 has not; after 8 certified ones two failures in a row keep three quarters
    (4 x 8 >= 3 x 10), a third does not (4 x 8 < 3 x 11)"""
    base = backbone(18, STRIPS_N)
    clean = [_b(substituted(base, 50 * i + 25)) for i in range(1, 9)]
    cut = _b(base[:150], base[450:])
    # (a second read of that kind would walk the bridge the first one left in the graph: the failures that follow are 100 nt of the base
    # and 200 nt of something else each)
    half = [_b(base[100 * i:100 * i + 100], backbone(180 + i, 200)) for i in (1, 3, 5)]
    b = _b(base)
    return {
        "strips_9th": {"pack": [b] + clean + [cut], "family": "strips", "back": None, "strips": 1},
        "strips_8th": {"pack": [b] + clean[:7] + [cut] + clean[7:], "family": "strips", "back": 8, "strips": 0},
        "strips_quarters_kept": {"pack": [b] + clean + half[:2], "family": "strips", "back": None, "strips": 2},
        "strips_quarters_lost": {"pack": [b] + clean + half, "family": "strips", "back": 11, "strips": 2},
    }


# ---- the score range of the band's int16 rows ----
def _score_cases():
    x = backbone(19, 2560)
    last = substituted(x, 2559)
    return {"score_12800": {"pack": [_b(x)] * 3, "family": "score", "S": [12800, 12800]},
            "score_last_column": {"pack": [_b(x), _b(x), _b(last)], "family": "score", "S": [12800, 12795]}}


def cases():
    """name -> case: "pack" and what the case claims about it"""
    out = {}
    for family in ("right", "diag", "left"):
        for cplb in LADDER:
            for variant in VARIANTS:
                out["%s_%d_%s" % (family, cplb, variant)] = _edge_case(family, cplb, variant)
    out.update(_clamp_cases())
    out.update(_skip_cases())
    out.update(_history_cases())
    out.update(_strips_cases())
    out.update(_score_cases())
    return out


# ---- the edge cases in small, for a DP in plain Python ----
def small_edge(family, N=64, d=4, t=8):
    """a right / left `on` case scaled down, against the chain of one base: (base, read, C, L, t, s)"""
    base = backbone(20 + (family == "left"), N)
    if family == "right":
        L = N
        read = np.concatenate([junk(base, 0, t), base[:N - t]])
        s = t
    else:
        L = N - d
        s = d + t
        read = np.concatenate([base[s:], junk(base, L - t, L)])
    return base, read, N, L, t, s
