"""The contract of `align_pairs` (include/rattle_hip.h) in plain Python, twice, and the cases the tests are built from.

Smith-Waterman, match +5, mismatch -4, gap -8 per gapped column (linear), letters A, C, G, T = U; a cell with H == 0 begins a new
alignment, predecessors that tie are taken diagonal, then up (a read base against a gap), then left (a transcript base against a gap);
the end cell is the largest H, ties to the smallest i, then the smallest j.

  traceback(q, t)   the classic form: the whole matrix, then a walk back from the end cell that counts every column it passes
  forward(q, t)     what kernel E does: (start_i, start_j, matches) carried with every cell's score, two rows at a time, the other
                    counts from the identity  mismatches = (8 (sq + st) - 21 M + S) / 12

Both return a record (FIELDS order) on the coordinates of the sequence they are handed; align() applies the strand and maps q_* back to
the read as given.  No device, no numpy in the recurrences."""
import numpy as np

MATCH, MISMATCH, GAP = 5, -4, -8
FIELDS = (("status", np.uint8), ("score", np.int32), ("q_start", np.uint32), ("q_end", np.uint32), ("t_start", np.uint32),
          ("t_end", np.uint32), ("matches", np.uint32), ("mismatches", np.uint32), ("q_gap", np.uint32), ("t_gap", np.uint32))
NONE = (1, 0, 0, 0, 0, 0, 0, 0, 0, 0)          # no positive cell, or an empty sequence
SKIPPED = (2, 0, 0, 0, 0, 0, 0, 0, 0, 0)       # len(q) * len(t) > max_cells
NOT_SUBMITTED = (3, 0, 0, 0, 0, 0, 0, 0, 0, 0)

_T = bytes.maketrans(b"U", b"T")
_RC = bytes.maketrans(b"ACGTU", b"TGCAA")


def revcomp(s: bytes) -> bytes:
    """A<->T, C<->G, U complements to A"""
    return s.translate(_RC)[::-1]


def fill(q: bytes, t: bytes):
    """the whole matrix H, (len(q) + 1) x (len(t) + 1), as a list of rows"""
    q, t = q.translate(_T), t.translate(_T)
    prev = [0] * (len(t) + 1)
    H = [prev]
    for qc in q:
        row = [0] * (len(t) + 1)
        left = 0
        for j, tc in enumerate(t, 1):
            d = prev[j - 1] + (MATCH if qc == tc else MISMATCH)
            u = prev[j] + GAP
            left += GAP
            h = d if d > u else u
            if left > h:
                h = left
            if h < 0:
                h = 0
            row[j] = left = h
        H.append(row)
        prev = row
    return H


def end_cell(H):
    """the largest H; ties: the smallest i, then the smallest j.  (0, 0, 0) if no cell is positive."""
    best, bi, bj = 0, 0, 0
    for i, row in enumerate(H):
        m = max(row)
        if m > best:
            best, bi, bj = m, i, row.index(m)
    return best, bi, bj


def walk(q: bytes, t: bytes, H, i: int, j: int, zero_rule: bool = True):
    """From cell (i, j) back to the cell where its alignment begins: the cells of the path, end first.  Each step takes the predecessor
    that reproduces the cell's score, diagonal, then up, then left.  zero_rule=False: a walk that does NOT stop at an interior zero (it
    goes on while some predecessor reproduces the score; the test of the zero-crossing case uses it to show what the rule is for)."""
    q, t = q.translate(_T), t.translate(_T)
    path = [(i, j)]
    while i > 0 and j > 0 and (H[i][j] > 0 or not zero_rule):
        h = H[i][j]
        if h == H[i - 1][j - 1] + (MATCH if q[i - 1] == t[j - 1] else MISMATCH):
            i, j = i - 1, j - 1
        elif h == H[i - 1][j] + GAP:
            i -= 1
        elif h == H[i][j - 1] + GAP:
            j -= 1
        else:
            break                              # (only a zero that no predecessor explains: the path begins here)
        path.append((i, j))
    return path


def traceback(q: bytes, t: bytes):
    """the classic form: fill, end cell, walk back, count the columns"""
    if not q or not t:
        return NONE
    H = fill(q, t)
    score, i, j = end_cell(H)
    if score <= 0:
        return NONE
    path = walk(q, t, H, i, j)
    qq, tt = q.translate(_T), t.translate(_T)
    M = X = qg = tg = 0
    for (a, b), (c, d) in zip(path, path[1:]):      # a step from (c, d) to (a, b)
        if a == c + 1 and b == d + 1:
            if qq[a - 1] == tt[b - 1]:
                M += 1
            else:
                X += 1
        elif a == c + 1:
            qg += 1
        else:
            tg += 1
    si, sj = path[-1]
    assert H[si][sj] == 0 and score == MATCH * M + MISMATCH * X + GAP * (qg + tg)
    return (0, score, si, i, sj, j, M, X, qg, tg)


def forward(q: bytes, t: bytes):
    """the forward-carried payload: no matrix, no walk"""
    if not q or not t:
        return NONE
    q, t = q.translate(_T), t.translate(_T)
    n = len(t)
    pH, pI, pJ, pM = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    best = (0, 0, 0, 0, 0, 0)                       # score, i, j, start_i, start_j, matches
    for i, qc in enumerate(q, 1):
        cH, cI, cJ, cM = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
        for j in range(1, n + 1):
            eq = qc == t[j - 1]
            d = pH[j - 1] + (MATCH if eq else MISMATCH)
            u = pH[j] + GAP
            l = cH[j - 1] + GAP
            h = max(0, d, u, l)
            if h == 0:
                continue                            # begins a new alignment: whatever continues from here takes its own coordinates
            if d >= u and d >= l:
                if pH[j - 1] == 0:
                    si, sj, m = i - 1, j - 1, 0
                else:
                    si, sj, m = pI[j - 1], pJ[j - 1], pM[j - 1]
                m += eq
            elif u >= l:
                si, sj, m = pI[j], pJ[j], pM[j]
            else:
                si, sj, m = cI[j - 1], cJ[j - 1], cM[j - 1]
            cH[j], cI[j], cJ[j], cM[j] = h, si, sj, m
            if h > best[0]:
                best = (h, i, j, si, sj, m)
        pH, pI, pJ, pM = cH, cI, cJ, cM
    S, i, j, si, sj, M = best
    if S <= 0:
        return NONE
    sq, st = i - si, j - sj
    X12 = 8 * (sq + st) - 21 * M + S
    assert X12 % 12 == 0 and X12 >= 0, (X12, sq, st, M, S)
    X = X12 // 12
    assert sq - M - X >= 0 and st - M - X >= 0
    return (0, S, si, i, sj, j, M, X, sq - M - X, st - M - X)


def align(q: bytes, t: bytes, rev: int = 0, form=traceback):
    """the record of one pair: the strand applied, q_* on the read as given"""
    r = form(revcomp(q) if rev else q, t)
    if rev and r[0] == 0:
        r = r[:2] + (len(q) - r[3], len(q) - r[2]) + r[4:]
    return r


_memo = {}


def records(targets, reads, target_of_read, rev, max_cells=0, form=traceback):
    """what rattle_hip_align_pairs returns: a dict of arrays (FIELDS).  Pairs are remembered, so tests that share a case share its
    reference."""
    out = []
    for q, x, s in zip(reads, target_of_read, rev):
        if x < 0:
            out.append(NOT_SUBMITTED)
            continue
        t = targets[x]
        if not q or not t:
            out.append(NONE)
        elif max_cells and len(q) * len(t) > max_cells:
            out.append(SKIPPED)
        else:
            key = (q, t, int(s), form.__name__)
            if key not in _memo:
                _memo[key] = align(q, t, int(s), form)
            out.append(_memo[key])
    return {f: np.array([r[k] for r in out], dt) for k, (f, dt) in enumerate(FIELDS)}


def same(got: dict, want: dict):
    """the differences between two record sets: [(field, read, got, want)]; empty = equal"""
    bad = []
    for f, dt in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.dtype != np.dtype(dt) or g.shape != w.shape:
            bad.append((f, -1, str(g.dtype), g.shape))
            continue
        bad += [(f, int(i), int(g[i]), int(w[i])) for i in np.nonzero(g != w)[0]]
    return bad


def cells(case):
    """the DP cells a case hands a reference"""
    targets, reads, target_of_read = case[0], case[1], case[2]
    return sum(len(q) * len(targets[x]) for q, x in zip(reads, target_of_read) if x >= 0)


# ---- case builders: (targets, reads, target_of_read, rev) ------------------------------------------------------------------------
def rnd(rng, n: int) -> bytes:
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def mutate(rng, s: bytes, rate: float) -> bytes:
    """substitutions, insertions and deletions, a third of `rate` each"""
    out = bytearray()
    for b in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            b = b"ACGT"[int(rng.integers(0, 4))]
        out.append(b)
        if rng.random() < rate / 3:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
    return bytes(out)


def pairs_case(pairs):
    """[(read, transcript, rev)] as one case: every pair its own target"""
    return [t for _, t, _ in pairs], [q for q, _, _ in pairs], list(range(len(pairs))), [s for _, _, s in pairs]


# the edges of kernel E as built: blocks of 64 rows (the strip is written from 65 rows on, read and written from 129), refills of 64 columns
EDGE_ROWS = (1, 63, 64, 65, 127, 128, 129)
EDGE_COLS = (1, 63, 64, 65, 127, 128, 129)


def edge_case(seed=11):
    """Every edge length of the read against every edge length of the transcript (each edge is met by both sequences): the read a
    mutated piece of a common ancestor, so that the alignment spans the block and refill edges."""
    rng = np.random.default_rng(seed)
    base = rnd(rng, 160)
    pairs = []
    for lq in EDGE_ROWS:
        for lt in EDGE_COLS:
            q = mutate(rng, base, 0.1)
            t = mutate(rng, base, 0.05)
            q = (q + rnd(rng, lq))[:lq]
            t = (t + rnd(rng, lt))[:lt]
            pairs.append((q, t, 0))
    return pairs_case(pairs)


def long_case(seed=12):
    """200 x 700 (four row blocks, eleven refills) and its transpose: the read lies in the middle of the transcript"""
    rng = np.random.default_rng(seed)
    t = rnd(rng, 700)
    q = (mutate(rng, t[260:470], 0.12) + rnd(rng, 200))[:200]
    return pairs_case([(q, t, 0), (t, q, 0)])


def tie_cases():
    """homopolymer and dinucleotide repeats of unequal length, a single deleted base inside a run"""
    rng = np.random.default_rng(13)
    a, b = rnd(rng, 30), rnd(rng, 30)
    return pairs_case([(b"A" * 40, b"A" * 47, 0), (b"A" * 47, b"A" * 40, 0), (b"AC" * 30, b"AC" * 33, 0), (b"AC" * 33, b"AC" * 30, 0),
                       (a + b"G" * 9 + b, a + b"G" * 10 + b, 0), (a + b"G" * 10 + b, a + b"G" * 9 + b, 0)])


def two_ends_cases():
    """the read twice in the transcript (the smallest j wins), the transcript twice in the read (the smallest i wins)"""
    rng = np.random.default_rng(14)
    x, f1, f2, f3 = rnd(rng, 50), rnd(rng, 20), rnd(rng, 31), rnd(rng, 17)
    return pairs_case([(x, f1 + x + f2 + x + f3, 0), (f1 + x + f2 + x + f3, x, 0)])


def zero_crossing_case():
    """4 matches, 5 mismatches, then 60 matches: 20 - 20 = 0 after the mismatches, the alignment begins behind them"""
    rng = np.random.default_rng(15)
    head, tail = b"ACGT", rnd(rng, 60)
    return pairs_case([(head + b"AAAAA" + tail, head + b"CCCCC" + tail, 0)])


def strand_case(seed=16):
    """reads written with U, reverse-complemented, on transcripts written with T; the aligned part is not centred in the read"""
    rng = np.random.default_rng(seed)
    pairs = []
    for lt, a, b, junk_front, junk_back in ((300, 40, 200, 70, 5), (150, 0, 150, 0, 33), (90, 10, 80, 12, 0)):
        t = rnd(rng, lt)
        q = rnd(rng, junk_front) + mutate(rng, t[a:b], 0.08) + rnd(rng, junk_back)      # on the transcript's strand ...
        q = revcomp(q).replace(b"T", b"U")                                              # ... as it was sequenced
        pairs.append((q, t, 1))
        pairs.append((q, t, 0))                                                         # (the wrong strand: little or nothing)
    return pairs_case(pairs)


def status_case():
    """AAAA on CCCC, an empty read, an empty transcript, a read that is not submitted, and one pair for max_cells (24 x 30 cells)"""
    rng = np.random.default_rng(17)
    t = rnd(rng, 30)
    targets = [b"CCCC", t, b""]
    reads = [b"AAAA", b"", t[3:27], t[3:27], t[3:27]]
    return targets, reads, [0, 1, 2, -1, 1], [0, 0, 0, 0, 0]


def random_case(seed=18, n=60):
    """reads cut from the transcript with 15 % errors, lengths 30 - 400, a third of them unrelated, both strands"""
    rng = np.random.default_rng(seed)
    targets = [rnd(rng, n) for n in (40, 64, 90, 128, 129, 150, 193, 230, 257, 300, 365, 400)]
    reads, tor, rev = [], [], []
    for i in range(n):
        x = int(rng.integers(0, len(targets)))
        t = targets[x]
        lq = 30 + int(370 * rng.random() ** 2)          # 30 .. 400, the short ones more often: the case stays below 2e6 cells
        if i % 3 == 2:
            q = rnd(rng, lq)
        else:                                        # (a read longer than its transcript: the whole transcript, then an overhang)
            a = int(rng.integers(0, max(0, len(t) - lq) + 1))
            q = mutate(rng, t[a:a + lq], 0.15)
            q += rnd(rng, max(0, lq - len(q)))
        s = int(rng.integers(0, 2))
        reads.append(revcomp(q) if s else q)
        tor.append(x)
        rev.append(s)
    return targets, reads, tor, rev


CASES = {"edges": edge_case, "long": long_case, "ties": tie_cases, "two_ends": two_ends_cases, "zero_crossing": zero_crossing_case,
         "strand": strand_case, "status": status_case, "random": random_case}
