"""Host-side mirror of the reference interface over the C ABI.

`Context.cluster_reads` has the argument meaning of cluster_reads
(/root/reference/cluster.hpp:44); `cluster_command` is the `rattle cluster` flow of
/root/reference/main.cpp:245-323 (length sort, gene level, optional --iso second level,
translation to original record indices).  Python is used here because this image has the
reference's C++ toolchain but the test harness is pytest; the C++ host with the same
structure is rattle_amd/csrc/rattle_main.cpp.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ClusterParams, ClusterSet, Correction, CorrectParams, MsaSet, check

K_KMER, K_FILTER, K_SCORE, K_POA, K_POST, K_ASSIGN, K_ALIGN, K_CIGAR = 0, 1, 2, 3, 4, 5, 6, 7
K_ALIGN_AFFINE, K_CIGAR_AFFINE = 8, 9          # the three-state forms of kernels E and F (align_pairs / align_cigars with a scoring)
K_ABUNDANCE = 10                               # the EM of Context.abundance (csrc/abundance.hip)
K_PILEUP = 11                                  # kernel G of Context.align_pileup (csrc/pair_pileup.hip)
ALIGN_MODES = {"local": 0, "read": 1}         # RATTLE_ALIGN_LOCAL, RATTLE_ALIGN_READ


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(C.POINTER(t))


def pack_reads(seqs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    cat = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy() if len(seqs) else np.zeros(0, np.uint8)
    return cat, off


@dataclass
class Clusters:
    main_id: np.ndarray
    main_rev: np.ndarray
    offsets: np.ndarray
    member_id: np.ndarray
    member_rev: np.ndarray
    counters: np.ndarray
    joins: Optional[dict] = None

    def report(self) -> Optional[dict]:
        """The cluster report: a dict of arrays with one entry per join (level, pass, bv_threshold, into, absorbed, rev, bases,
        hc_bases, min_len, score, variance; include/rattle_hip.h), or None if the set was made with the report off
        (Context.set_cluster_report)."""
        return self.joins

    def as_list(self):
        """[( (main_id, main_rev, -1), [(id, rev, -1), ...] ), ...] like rattle_amd.hps."""
        out = []
        for c in range(len(self.main_id)):
            a, b = int(self.offsets[c]), int(self.offsets[c + 1])
            out.append(((int(self.main_id[c]), int(self.main_rev[c]), -1),
                        [(int(self.member_id[i]), int(self.member_rev[i]), -1) for i in range(a, b)]))
        return out


def msa_pack(rows: Sequence[bytes], quals: Optional[Sequence[bytes]] = None):
    """MSA rows (bytes of one length, '-' for gaps) as a pack of Context.debug_post_msa: (width, sequences, the MSA column of
    every base, qualities)."""
    width = len(rows[0]) if len(rows) else 0
    assert all(len(r) == width for r in rows)
    mat = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), width)
    cols = [np.nonzero(m != ord("-"))[0].astype(np.uint32) for m in mat]
    seqs = [m[c].tobytes() for m, c in zip(mat, cols)]
    assert quals is None or all(len(q) == len(s) for q, s in zip(quals, seqs))
    return width, seqs, cols, None if quals is None else list(quals)


def correct_params(min_occ=0.3, gap_occ=0.3, err_ratio=30.0, split=200, min_reads=5, n_threads=0, vote_order: bytes = b"",
                   pack_order=None, max_pack_cells=0):
    """rattle_correct_params; pack_order = {cluster: [pack indices in the order their consensi enter POA #3]}.
    Returns (struct, keep-alive list)."""
    P = CorrectParams(min_occ, gap_occ, err_ratio, split, min_reads, n_threads, vote_order)
    keep = []
    if pack_order:
        cl = np.array(sorted(pack_order), np.uint32)
        offs = np.zeros(len(cl) + 1, np.uint32)
        offs[1:] = np.cumsum([len(pack_order[int(c)]) for c in cl])
        perm = np.array([x for c in cl for x in pack_order[int(c)]], np.uint32)
        P.n_pack_orders = len(cl)
        P.pack_order_cluster = _ptr(cl, C.c_uint32); P.pack_order_offsets = _ptr(offs, C.c_uint32); P.pack_order_perm = _ptr(perm, C.c_uint32)
        keep = [cl, offs, perm]
    P.max_pack_cells = int(max_pack_cells)
    return P, keep


def cluster_report(lib, ptr) -> Optional[dict]:
    """The cluster report of a library-owned rattle_cluster_set (pointer) as a dict of arrays, one entry per join
    (_lib.CLUSTER_REPORT_FIELDS); None if the set was made with the report off (Context.set_cluster_report)."""
    out = C.POINTER(_lib.ClusterReport)()
    rc = lib.rattle_hip_cluster_report(ptr, C.byref(out))
    if rc == _lib.RATTLE_ERR_STATE:
        return None
    check(rc)
    n = int(out.contents.n)
    res = {f: np.ctypeslib.as_array(getattr(out.contents, f), (max(n, 1),))[:n].copy() for f, _ in _lib.CLUSTER_REPORT_FIELDS}
    lib.rattle_hip_cluster_report_free(out)
    return res


def concat_reports(parts: Sequence[dict]) -> dict:
    """cluster reports one after the other"""
    return {f: np.concatenate([p[f] for p in parts]) if parts else np.zeros(0, np.dtype(t)) for f, t in _lib.CLUSTER_REPORT_FIELDS}


def correction_report(lib, ptr) -> Optional[dict]:
    """The correction report of a library-owned rattle_correction (pointer) as a dict of uint32 arrays, one entry per record of
    `corrected` (_lib.REPORT_FIELDS); None if the correction was made with the report off (Context.set_correction_report)."""
    out = C.POINTER(_lib.CorrectionReport)()
    rc = lib.rattle_hip_correction_report(ptr, C.byref(out))
    if rc == _lib.RATTLE_ERR_STATE:
        return None
    check(rc)
    n = out.contents.n
    res = {f: np.ctypeslib.as_array(getattr(out.contents, f), (max(n, 1),))[:n].copy() for f in _lib.REPORT_FIELDS}
    lib.rattle_hip_correction_report_free(out)
    return res


def consensus_support(lib, ptr) -> Optional[dict]:
    """The consensus support of a library-owned rattle_correction (pointer) as a dict of arrays: level (uint8, per record of
    `consensi`), off (uint64, [n + 1], == consensi.off) and support, depth, pack_support, pack_depth (uint32, per base); None if the
    correction was made with the support off (Context.set_consensus_support)."""
    out = C.POINTER(_lib.ConsensusSupport)()
    rc = lib.rattle_hip_consensus_support(ptr, C.byref(out))
    if rc == _lib.RATTLE_ERR_STATE:
        return None
    check(rc)
    S = out.contents
    n = int(S.n)
    res = {"level": np.ctypeslib.as_array(S.level, (max(n, 1),))[:n].copy(), "off": np.ctypeslib.as_array(S.off, (n + 1,)).copy()}
    tot = int(res["off"][n])
    res.update({f: np.ctypeslib.as_array(getattr(S, f), (max(tot, 1),))[:tot].copy() for f in _lib.SUPPORT_FIELDS})
    lib.rattle_hip_consensus_support_free(out)
    return res


def support_tsv(names: Sequence[bytes], n_reads: Sequence[int], sup: dict) -> bytes:
    """consensus_support.tsv as `rattle correct --support` writes it: one line per consensus (names: the first token of its header,
    n_reads: its `reads=`): consensus, length, level, reads, min_ratio (the smallest support / depth, %.17g), weak (bases with
    2 * support <= depth), support and depth as comma-separated per-base lists."""
    lines = [b"consensus\tlength\tlevel\treads\tmin_ratio\tweak\tsupport\tdepth\n"]
    for i, name in enumerate(names):
        a, b = int(sup["off"][i]), int(sup["off"][i + 1])
        s, d = sup["support"][a:b], sup["depth"][a:b]
        ratio = float(np.min(s.astype(np.float64) / d.astype(np.float64))) if b > a else 0.0
        lines.append(b"%s\t%d\t%d\t%d\t%s\t%d\t%s\t%s\n" % (name, b - a, int(sup["level"][i]), int(n_reads[i]), ("%.17g" % ratio).encode(),
                                                             int(np.sum(2 * s.astype(np.uint64) <= d)), ",".join(map(str, s)).encode(),
                                                             ",".join(map(str, d)).encode()))
    return b"".join(lines)


def unpack_correction(R) -> dict:
    """rattle_correction (the struct or a pointer to it) -> dict of record lists (read_id, cluster_id, n_reads, seq, qual), counters,
    skip list and, when the correction carries one, the correction report under "report" (a dict of uint32 arrays parallel to
    "corrected") and the consensus support under "support" (consensus_support).  Both live behind the library's own object, so they
    are found for `ptr.contents` of a result the library returned, not for a copy of the struct."""
    if hasattr(R, "contents"):
        R = R.contents
    def unpack(S):
        n = S.n
        o = np.ctypeslib.as_array(S.off, (n + 1,)).copy()
        tot = int(o[n])
        sq = C.string_at(S.seq, tot); ql = C.string_at(S.qual, tot)
        rid = np.ctypeslib.as_array(S.read_id, (max(n, 1),))[:n]
        cid = np.ctypeslib.as_array(S.cluster_id, (max(n, 1),))[:n]
        nr = np.ctypeslib.as_array(S.n_reads, (max(n, 1),))[:n]
        return [(int(rid[i]), int(cid[i]), int(nr[i]), sq[int(o[i]):int(o[i + 1])], ql[int(o[i]):int(o[i + 1])])
                for i in range(n)]

    K = R.skipped
    skipped = []
    if K.n:
        ro = np.ctypeslib.as_array(K.read_off, (K.n + 1,))
        rid = np.ctypeslib.as_array(K.read_id, (max(int(ro[K.n]), 1),))
        for i in range(K.n):
            skipped.append({"cluster": int(K.cluster_id[i]), "pack": int(K.pack[i]), "stage": int(K.stage[i]),
                            "reads": [int(x) for x in rid[int(ro[i]):int(ro[i + 1])]]})
    res = {"corrected": unpack(R.corrected), "uncorrected": unpack(R.uncorrected), "consensi": unpack(R.consensi),
           "counters": np.array(list(R.counters), dtype=np.uint64), "skipped": skipped}
    support = consensus_support(_lib.load(), C.pointer(R))
    if support is not None:
        res["support"] = support
    report = correction_report(_lib.load(), C.pointer(R))
    if report is not None:
        res["report"] = report
    return res


def correction_digest(R) -> int:
    """CRC over every output array of a rattle_correction (ids, offsets, bases, qualities)."""
    import zlib
    crc = 0
    for S in (R.corrected, R.uncorrected, R.consensi):
        n = S.n
        o = np.ctypeslib.as_array(S.off, (n + 1,))
        tot = int(o[n])
        crc = zlib.crc32(o.tobytes(), crc)
        for arr in (S.read_id, S.cluster_id, S.n_reads):
            crc = zlib.crc32(np.ctypeslib.as_array(arr, (max(n, 1),))[:n].tobytes(), crc)
        crc = zlib.crc32(C.string_at(S.seq, tot), crc)
        crc = zlib.crc32(C.string_at(S.qual, tot), crc)
    return crc


class CorrectionHandle:
    """A library-owned rattle_correction kept alive by the caller (bench.py digests it outside the timed region)."""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def counts(self):
        if self.ptr is None:
            return (0, 0, 0, np.zeros(8, np.uint64))
        R = self.ptr.contents
        return (R.corrected.n, R.uncorrected.n, R.consensi.n, np.array(list(R.counters), dtype=np.uint64))

    def digest(self):
        return None if self.ptr is None else correction_digest(self.ptr.contents)

    def report(self):
        """The per-read correction report: a dict of uint32 arrays parallel to the corrected records (in_len, out_len, trim_front,
        trim_back, match, substituted, mismatch_kept, inserted, deleted, gap_kept).  Raises if the correction was made with the
        report off (Context.set_correction_report)."""
        if self.ptr is None:
            raise _lib.RattleError("no correction on this rank")
        lib = self.lib or _lib.load()
        res = correction_report(lib, self.ptr)
        if res is None:
            raise _lib.RattleError(f"librattle_hip error {_lib.RATTLE_ERR_STATE}: {lib.rattle_hip_last_error().decode()}")
        return res

    def support(self):
        """The consensus support (consensus_support): a dict of arrays, or None if the correction was made with the support off
        (Context.set_consensus_support)."""
        if self.ptr is None:
            return None
        return consensus_support(self.lib or _lib.load(), self.ptr)

    def host_bytes(self):
        """bases + qualities held by the three read sets (what free() gives back to the OS)"""
        if self.ptr is None:
            return 0
        R = self.ptr.contents
        tot = 0
        for S in (R.corrected, R.uncorrected, R.consensi):
            if S.n:
                tot += 2 * int(np.ctypeslib.as_array(S.off, (S.n + 1,))[S.n])
        return tot

    def free(self):
        if self.ptr is not None:
            self.lib.rattle_hip_correction_free(self.ptr)
            self.ptr = None


class Context:
    """One HIP device + the device-resident read index (rattle_ctx)."""

    def __init__(self, device: Optional[int] = 0):
        """device=None: a host-only context (exchange entry points only, rattle_hip_ctx_create_host)."""
        self.lib = _lib.load()
        h = C.c_void_p()
        if device is None:
            check(self.lib.rattle_hip_ctx_create_host(C.byref(h)))
        else:
            check(self.lib.rattle_hip_ctx_create(device, C.byref(h)))
        self.h = h
        self.n = 0
        self.both = False
        self.k = 0
        self.cluster_report = False
        self.consensus_support = False

    def close(self):
        if self.h:
            self.lib.rattle_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_cluster_report(self, on: bool):
        """Switch the cluster report of the following cluster_* calls (and the evidence debug_evaluate returns) on or off (off by
        default): Clusters.report() of their results."""
        check(self.lib.rattle_hip_set_cluster_report(self.h, int(bool(on))))
        self.cluster_report = bool(on)

    def set_correction_report(self, on: bool):
        """Switch the per-read correction report of the following correct_* / debug_post_msa calls on or off (off by default)."""
        check(self.lib.rattle_hip_set_correction_report(self.h, int(bool(on))))

    def set_consensus_support(self, on: bool):
        """Switch the per-base support of the consensi of the following correct_* calls (and what debug_consensus_support returns) on
        or off (off by default): CorrectionHandle.support(), the "support" key of correct_reads."""
        check(self.lib.rattle_hip_set_consensus_support(self.h, int(bool(on))))
        self.consensus_support = bool(on)

    # a3
    def load_reads(self, seqs: Sequence[bytes], k: int, both_strands: bool):
        cat, off = pack_reads(seqs)
        self.load_packed(cat, off, k, both_strands)

    def stage_reads(self, cat: np.ndarray, qcat: Optional[np.ndarray], off: np.ndarray):
        """Keep the reads (and qualities) resident in HBM; later calls given the same arrays skip the upload."""
        q = _ptr(qcat, C.c_uint8) if qcat is not None else None
        check(self.lib.rattle_hip_stage_reads(self.h, _ptr(cat, C.c_uint8), q, _ptr(off, C.c_uint64), len(off) - 1))

    def unstage_reads(self):
        check(self.lib.rattle_hip_unstage_reads(self.h))

    def load_packed(self, cat: np.ndarray, off: np.ndarray, k: int, both_strands: bool):
        n = len(off) - 1
        check(self.lib.rattle_hip_load_reads(self.h, _ptr(cat, C.c_uint8), _ptr(off, C.c_uint64), n, k, int(both_strands)))
        self.n, self.both, self.k = n, bool(both_strands), k
        self._lens = (off[1:] - off[:-1]).astype(np.int64)

    def read_index(self, r: int, strand: int):
        nk = max(int(self._lens[r]) - self.k, 0)
        h = np.zeros(nk, np.uint32)
        p = np.zeros(nk, np.int32)
        bv = np.zeros(64, np.uint64)
        pc = C.c_uint32()
        check(self.lib.rattle_hip_get_read_index(self.h, r, strand, _ptr(h, C.c_uint32), _ptr(p, C.c_int32),
                                                 _ptr(bv, C.c_uint64), C.byref(pc)))
        return h, p, bv, pc.value

    # a4
    def bv_filter(self, seed_ids, cand_ids, first_cand, lut, fwd_bypass: bool) -> np.ndarray:
        s = np.ascontiguousarray(seed_ids, np.uint32)
        c = np.ascontiguousarray(cand_ids, np.uint32)
        f = np.ascontiguousarray(first_cand, np.uint32)
        l = np.ascontiguousarray(lut, np.uint16)
        assert len(l) == 4097 and len(f) == len(s)
        out = np.zeros((len(s), len(c)), np.uint8)
        check(self.lib.rattle_hip_bv_filter(self.h, _ptr(s, C.c_uint32), len(s), _ptr(c, C.c_uint32), len(c),
                                            _ptr(f, C.c_uint32), _ptr(l, C.c_uint16), int(fwd_bypass), _ptr(out, C.c_uint8)))
        return out

    # a5-a7
    def pair_score(self, i_ids, j_ids, strand):
        i = np.ascontiguousarray(i_ids, np.uint32)
        j = np.ascontiguousarray(j_ids, np.uint32)
        s = np.ascontiguousarray(strand, np.uint8)
        n = len(i)
        bases = np.zeros(n, np.int32); hc = np.zeros(n, np.int32); nd = np.zeros(n, np.int32)
        nm = np.zeros(n, np.int32); var = np.zeros(n, np.float64)
        check(self.lib.rattle_hip_pair_score(self.h, _ptr(i, C.c_uint32), _ptr(j, C.c_uint32), _ptr(s, C.c_uint8), n,
                                             _ptr(bases, C.c_int32), _ptr(hc, C.c_int32), _ptr(nd, C.c_int32),
                                             _ptr(var, C.c_double), _ptr(nm, C.c_int32)))
        return bases, hc, nd, var, nm

    # a8-a11
    def cluster_reads(self, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, min_bv_threshold=0.2, bv_falloff=0.05,
                      min_reads_cluster=0, use_hc=False, repr_percentile=0.15, is_rna=False,
                      subset: Optional[np.ndarray] = None) -> Clusters:
        P = ClusterParams(t_s, t_v, bv_threshold, min_bv_threshold, bv_falloff, min_reads_cluster, int(use_hc),
                          repr_percentile, int(is_rna))
        out = C.POINTER(ClusterSet)()
        if subset is None:
            check(self.lib.rattle_hip_cluster_reads(self.h, C.byref(P), C.byref(out)))
        else:
            sub = np.ascontiguousarray(subset, np.uint32)
            check(self.lib.rattle_hip_cluster_subset(self.h, C.byref(P), _ptr(sub, C.c_uint32), len(sub), C.byref(out)))
        return self._take_clusters(out)

    def cluster_subsets(self, subsets: Sequence[np.ndarray], t_s=0.2, t_v=1000000.0, bv_threshold=0.4, min_bv_threshold=0.2,
                        bv_falloff=0.05, repr_percentile=0.15, is_rna=False, n_workers=0) -> List[Clusters]:
        """cluster_reads restricted to each subset (ids in processing order), all subsets in one call."""
        P = ClusterParams(t_s, t_v, bv_threshold, min_bv_threshold, bv_falloff, 0, 0, repr_percentile, int(is_rna))
        n = len(subsets)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([len(x) for x in subsets])
        ids = np.concatenate([np.asarray(x, np.uint32) for x in subsets]) if n and offs[n] else np.zeros(1, np.uint32)
        outs = (C.POINTER(ClusterSet) * max(n, 1))()
        check(self.lib.rattle_hip_cluster_subsets(self.h, C.byref(P), _ptr(ids, C.c_uint32), _ptr(offs, C.c_uint64), n, outs, n_workers))
        return [self._take_clusters(outs[i]) for i in range(n)]

    def _take_clusters(self, out) -> Clusters:
        cs = out.contents
        nc = cs.n_clusters
        offsets = np.ctypeslib.as_array(cs.offsets, (nc + 1,)).copy()
        nm = int(offsets[nc])
        res = Clusters(np.ctypeslib.as_array(cs.main_id, (max(nc, 1),))[:nc].copy(),
                       np.ctypeslib.as_array(cs.main_rev, (max(nc, 1),))[:nc].copy(), offsets,
                       np.ctypeslib.as_array(cs.member_id, (max(nm, 1),))[:nm].copy(),
                       np.ctypeslib.as_array(cs.member_rev, (max(nm, 1),))[:nm].copy(),
                       np.array(list(cs.counters), dtype=np.uint64), cluster_report(self.lib, out))
        self.lib.rattle_hip_cluster_set_free(out)
        return res

    def cluster_unsorted_packed(self, cat: np.ndarray, off: np.ndarray, k=10, t_s=0.2, t_v=1000000.0, bv_threshold=0.4,
                                min_bv_threshold=0.2, bv_falloff=0.05, repr_percentile=0.15, is_rna=False) -> Clusters:
        """main.cpp:254-277 on packed arrays in file order; ids in the result index the caller's order."""
        P = ClusterParams(t_s, t_v, bv_threshold, min_bv_threshold, bv_falloff, 0, 0, repr_percentile, int(is_rna))
        out = C.POINTER(ClusterSet)()
        check(self.lib.rattle_hip_cluster_unsorted(self.h, _ptr(cat, C.c_uint8), _ptr(off, C.c_uint64), len(off) - 1, k,
                                                   C.byref(P), C.byref(out)))
        return self._take_clusters(out)

    def cluster_iso_unsorted_packed(self, cat: np.ndarray, off: np.ndarray, k=10, iso_k=11, t_s=0.2, t_v=1000000.0, iso_t_s=0.3,
                                    iso_t_v=25.0, bv_threshold=0.4, min_bv_threshold=0.2, bv_falloff=0.05, repr_percentile=0.15,
                                    is_rna=False):
        """`rattle cluster --iso` (main.cpp:254-323) on packed arrays in file order.  Returns (Clusters, gene_id per
        cluster, number of gene clusters)."""
        P = ClusterParams(t_s, t_v, bv_threshold, min_bv_threshold, bv_falloff, 0, 0, repr_percentile, int(is_rna))
        Q = ClusterParams(iso_t_s, iso_t_v, bv_threshold, min_bv_threshold, bv_falloff, 0, 0, repr_percentile, int(is_rna))
        out = C.POINTER(ClusterSet)()
        ng = C.c_uint32()
        check(self.lib.rattle_hip_cluster_iso_unsorted(self.h, _ptr(cat, C.c_uint8), _ptr(off, C.c_uint64), len(off) - 1, k, iso_k,
                                                       C.byref(P), C.byref(Q), C.byref(out), C.byref(ng)))
        nc = out.contents.n_clusters
        gid = np.ctypeslib.as_array(out.contents.gene_id, (max(nc, 1),))[:nc].copy()
        return self._take_clusters(out), gid, ng.value

    def correct_packed(self, cat: np.ndarray, qcat: np.ndarray, off: np.ndarray, cl: Clusters, min_occ=0.3, gap_occ=0.3,
                       split=200, min_reads=5, n_threads=0, vote_order: bytes = b"", digest: bool = False, max_pack_cells=0,
                       gather_root: Optional[int] = None, keep: bool = False):
        """correct_reads on packed arrays; returns (n_corrected, n_uncorrected, n_consensi, counters)
        without materialising Python objects (the library still builds every output record).
        digest=True appends a CRC over every output array (ids, offsets, bases, qualities).
        gather_root: with several ranks, reassemble the sharded result on that rank
        (rattle_hip_correction_gather); the other ranks get zero counts and digest None.
        keep=True returns a CorrectionHandle instead (counts now, digest / free later)."""
        P, keep_alive = correct_params(min_occ, gap_occ, 30.0, split, min_reads, n_threads, vote_order, None, max_pack_cells)
        out = C.POINTER(Correction)()
        mid = cl.member_id if len(cl.member_id) else np.zeros(1, np.int32)
        mrev = cl.member_rev if len(cl.member_rev) else np.zeros(1, np.uint8)
        check(self.lib.rattle_hip_correct_reads(self.h, _ptr(cat, C.c_uint8), _ptr(qcat, C.c_uint8), _ptr(off, C.c_uint64),
                                                len(off) - 1, len(cl.main_id), _ptr(cl.offsets, C.c_uint32),
                                                _ptr(mid, C.c_int32), _ptr(mrev, C.c_uint8), C.byref(P), C.byref(out)))
        final = out
        if gather_root is not None:
            merged = C.POINTER(Correction)()
            check(self.lib.rattle_hip_correction_gather(self.h, out, gather_root, C.byref(merged)))
            self.lib.rattle_hip_correction_free(out)
            final = merged
        h = CorrectionHandle(self.lib, final if final else None)
        if keep:
            return h
        res = h.counts()
        if digest:
            res = res + (h.digest(),)
        h.free()
        return res

    # a15
    def poa_msa(self, packs: Sequence[Sequence[bytes]]):
        """MSA rows (list of bytes) for each pack of sequences."""
        flat = [s for p in packs for s in p]
        cat, off = pack_reads(flat)
        first = np.zeros(len(packs) + 1, np.uint32)
        first[1:] = np.cumsum([len(p) for p in packs])
        out = C.POINTER(MsaSet)()
        check(self.lib.rattle_hip_poa_msa(self.h, _ptr(cat, C.c_uint8), _ptr(off, C.c_uint64), len(flat),
                                          _ptr(first, C.c_uint32), len(packs), C.byref(out)))
        ms = out.contents
        ro = np.ctypeslib.as_array(ms.row_offset, (len(flat) + 1,)).copy()
        width = np.ctypeslib.as_array(ms.width, (max(len(packs), 1),))[:len(packs)].copy()
        total = int(ro[len(flat)])
        raw = C.string_at(ms.rows, total) if total else b""
        counters = np.array(list(ms.counters), dtype=np.uint64)
        self.lib.rattle_hip_msa_set_free(out)
        res = []
        q = 0
        for pi, p in enumerate(packs):
            rows = []
            for _ in p:
                rows.append(raw[int(ro[q]):int(ro[q + 1])])
                q += 1
            res.append(rows)
        return res, width, counters

    # a14-a20
    def correct_reads(self, seqs: Sequence[bytes], quals: Sequence[bytes], clusters, min_occ=0.3, gap_occ=0.3,
                      err_ratio=30.0, split=200, min_reads=5, n_threads=0, vote_order: bytes = b"", pack_order=None,
                      max_pack_cells=0, gather_root: Optional[int] = None):
        """correct_reads (correct.hpp:44).  `clusters` in rattle_amd.hps list form (ids index `seqs`).
        Returns dict of three record lists: (read_id, cluster_id, n_reads, seq, qual), the counters and
        the list of skipped packs.  With several ranks and gather_root set, the root gets the merged
        result and the others None."""
        cat, off = pack_reads(seqs)
        qcat, qoff = pack_reads(quals)
        assert np.array_equal(off, qoff), "sequence and quality lengths differ"
        coff = np.zeros(len(clusters) + 1, np.uint32)
        coff[1:] = np.cumsum([len(m) for _, m in clusters])
        mid = np.array([s[0] for _, m in clusters for s in m], np.int32)
        mrev = np.array([s[1] for _, m in clusters for s in m], np.uint8)
        if len(mid) == 0:
            mid = np.zeros(1, np.int32); mrev = np.zeros(1, np.uint8)
        P, keep = correct_params(min_occ, gap_occ, err_ratio, split, min_reads, n_threads, vote_order, pack_order, max_pack_cells)
        out = C.POINTER(Correction)()
        check(self.lib.rattle_hip_correct_reads(self.h, _ptr(cat, C.c_uint8), _ptr(qcat, C.c_uint8), _ptr(off, C.c_uint64),
                                                len(seqs), len(clusters), _ptr(coff, C.c_uint32), _ptr(mid, C.c_int32),
                                                _ptr(mrev, C.c_uint8), C.byref(P), C.byref(out)))
        final = out
        if gather_root is not None:
            merged = C.POINTER(Correction)()
            check(self.lib.rattle_hip_correction_gather(self.h, out, gather_root, C.byref(merged)))
            self.lib.rattle_hip_correction_free(out)
            final = merged
        if not final:
            return None
        res = unpack_correction(final.contents)
        self.lib.rattle_hip_correction_free(final)
        return res

    # ---- one job over several GPUs (include/rattle_hip.h, "One job over the GPUs of a node")
    def set_exchange_gloo(self, group=None):
        """Host-buffer all-gather through torch.distributed (any backend that takes CPU tensors, e.g. gloo)."""
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def fn(user, send, send_bytes, recv, recv_bytes):
            try:
                sizes = [int(recv_bytes[r]) for r in range(world)]
                mine = torch.frombuffer(C.string_at(send, send_bytes) if send_bytes else b"\0", dtype=torch.uint8)[:send_bytes].clone()
                pad = max(sizes + [1])
                buf = torch.zeros(pad, dtype=torch.uint8)
                buf[:send_bytes] = mine
                parts = [torch.zeros(pad, dtype=torch.uint8) for _ in range(world)]
                dist.all_gather(parts, buf, group=group)
                at = 0
                for r in range(world):
                    if sizes[r]:
                        C.memmove(recv + at, parts[r].numpy().ctypes.data, sizes[r])
                    at += sizes[r]
                return 0
            except Exception as e:  # never unwind through the C frame
                import sys
                print(f"exchange callback failed: {e}", file=sys.stderr)
                return 1

        self._xchg_fn = _lib.ALLGATHERV_FN(fn)       # keep the thunk alive
        check(self.lib.rattle_hip_set_exchange(self.h, rank, world, self._xchg_fn, None))

    def comm_init_rccl(self, group=None):
        """RCCL communicator for this context; the unique id travels through torch.distributed."""
        import torch
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        uid = np.zeros(128, np.uint8)
        if rank == 0:
            check(self.lib.rattle_hip_comm_unique_id(_ptr(uid, C.c_uint8)))
        dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
        t = torch.from_numpy(uid).to(dev)
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        uid = t.cpu().numpy().copy()
        check(self.lib.rattle_hip_comm_init(self.h, rank, world, _ptr(uid, C.c_uint8)))

    def comm_destroy(self):
        check(self.lib.rattle_hip_comm_destroy(self.h))

    def comm_probe(self):
        """Collective self-test of the attached transport (all ranks)."""
        check(self.lib.rattle_hip_comm_probe(self.h))

    def comm_stats(self):
        a = C.c_uint64(); b = C.c_uint64()
        check(self.lib.rattle_hip_comm_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # assign
    def _take_assignment(self, out) -> dict:
        n = int(out.contents.n)
        res = {f: np.ctypeslib.as_array(getattr(out.contents, f), (max(n, 1),))[:n].copy() for f, _ in _lib.ASSIGN_FIELDS}
        self.lib.rattle_hip_assignment_free(out)
        return res

    def assign_loaded(self, target_ids, read_ids, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, use_hc=False, is_rna=False,
                      target_batch=0, count_pass="auto") -> dict:
        """The loaded reads `read_ids` placed on the loaded reads `target_ids` by their best cluster_together score
        (rattle_hip_assign_loaded).  Returns a dict of arrays with one entry per read (_lib.ASSIGN_FIELDS): target (index into
        target_ids, -1: unassigned), rev, bases, hc_bases, min_len, score, variance, second_score (-1.0: no other target accepts),
        n_accepted.  count_pass as for debug_evaluate."""
        P = _lib.AssignParams(t_s, t_v, bv_threshold, int(use_hc), int(is_rna), int(target_batch), 0,
                              {"auto": 0, "seed": 1, "search": 2, "index": 3}[count_pass])
        t = np.ascontiguousarray(target_ids, np.uint32)
        r = np.ascontiguousarray(read_ids, np.uint32)
        out = C.POINTER(_lib.Assignment)()
        check(self.lib.rattle_hip_assign_loaded(self.h, C.byref(P), _ptr(t, C.c_uint32) if len(t) else None, len(t),
                                                _ptr(r, C.c_uint32) if len(r) else None, len(r), C.byref(out)))
        return self._take_assignment(out)

    def assign(self, targets: Sequence[bytes], reads: Sequence[bytes], k=10, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, use_hc=False,
               is_rna=False, target_batch=0, read_chunk=0, count_pass="auto") -> dict:
        """`reads` placed on `targets` (rattle_hip_assign_reads): both in any order, the reads indexed read_chunk at a time together
        with the targets (this replaces the context's loaded reads).  The result as for assign_loaded, target = index into `targets`."""
        P = _lib.AssignParams(t_s, t_v, bv_threshold, int(use_hc), int(is_rna), int(target_batch), int(read_chunk),
                              {"auto": 0, "seed": 1, "search": 2, "index": 3}[count_pass])
        tcat, toff = pack_reads(targets)
        rcat, roff = pack_reads(reads)
        return self.assign_packed(tcat, toff, rcat, roff, k, P)

    def assign_packed(self, tcat: np.ndarray, toff: np.ndarray, rcat: np.ndarray, roff: np.ndarray, k=10, params=None) -> dict:
        """assign() on packed arrays (pack_reads); params: an _lib.AssignParams, None = the defaults of assign()."""
        P = params if params is not None else _lib.AssignParams(0.2, 1000000.0, 0.4, 0, 0, 0, 0, 0)
        out = C.POINTER(_lib.Assignment)()
        check(self.lib.rattle_hip_assign_reads(self.h, _ptr(tcat, C.c_uint8) if len(tcat) else None, _ptr(toff, C.c_uint64), len(toff) - 1,
                                               _ptr(rcat, C.c_uint8) if len(rcat) else None, _ptr(roff, C.c_uint64), len(roff) - 1, k,
                                               C.byref(P), C.byref(out)))
        self.n = self.k = 0               # the loaded read set was replaced by the last chunk's
        return self._take_assignment(out)

    # assign with the candidate list
    def _take_candidates(self, cands) -> dict:
        n, k = int(cands.contents.n), int(cands.contents.k)
        res = {"count": np.ctypeslib.as_array(cands.contents.count, (max(n, 1),))[:n].copy()}
        for f, _ in _lib.CANDIDATE_FIELDS:
            res[f] = np.ctypeslib.as_array(getattr(cands.contents, f), (max(n * k, 1),))[:n * k].copy().reshape(n, k)
        self.lib.rattle_hip_candidates_free(cands)
        return res

    def assign_loaded_top(self, target_ids, read_ids, top, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, use_hc=False, is_rna=False,
                          target_batch=0, count_pass="auto"):
        """assign_loaded(), and the `top` (1..8) best targets of every read (rattle_hip_assign_loaded_top).  Returns (assignment,
        candidates): the dict assign_loaded returns for the same arguments, and a dict with "count" [n] -- min(top, accepting
        targets) -- and one [n, top] array per field of _lib.CANDIDATE_FIELDS: slot [r, j] is read r's j-th best target (one candidate
        per target, its better strand, forward on a tie; score descending, ties to the lower target index).  Slots j >= count[r] hold
        target -1, score -1.0 and zeros.  Slot 0 is the assignment's record."""
        P = _lib.AssignParams(t_s, t_v, bv_threshold, int(use_hc), int(is_rna), int(target_batch), 0,
                              {"auto": 0, "seed": 1, "search": 2, "index": 3}[count_pass])
        t = np.ascontiguousarray(target_ids, np.uint32)
        r = np.ascontiguousarray(read_ids, np.uint32)
        out = C.POINTER(_lib.Assignment)()
        cands = C.POINTER(_lib.Candidates)()
        check(self.lib.rattle_hip_assign_loaded_top(self.h, C.byref(P), _ptr(t, C.c_uint32) if len(t) else None, len(t),
                                                    _ptr(r, C.c_uint32) if len(r) else None, len(r), int(top), C.byref(out), C.byref(cands)))
        return self._take_assignment(out), self._take_candidates(cands)

    def assign_top(self, targets: Sequence[bytes], reads: Sequence[bytes], top, k=10, t_s=0.2, t_v=1000000.0, bv_threshold=0.4,
                   use_hc=False, is_rna=False, target_batch=0, read_chunk=0, count_pass="auto"):
        """assign(), and the `top` best targets of every read (rattle_hip_assign_reads_top): (assignment, candidates) as for
        assign_loaded_top, targets as indices into `targets`."""
        P = _lib.AssignParams(t_s, t_v, bv_threshold, int(use_hc), int(is_rna), int(target_batch), int(read_chunk),
                              {"auto": 0, "seed": 1, "search": 2, "index": 3}[count_pass])
        tcat, toff = pack_reads(targets)
        rcat, roff = pack_reads(reads)
        return self.assign_packed_top(tcat, toff, rcat, roff, top, k, P)

    def assign_packed_top(self, tcat: np.ndarray, toff: np.ndarray, rcat: np.ndarray, roff: np.ndarray, top, k=10, params=None):
        """assign_top() on packed arrays (pack_reads); params: an _lib.AssignParams, None = the defaults of assign()."""
        P = params if params is not None else _lib.AssignParams(0.2, 1000000.0, 0.4, 0, 0, 0, 0, 0)
        out = C.POINTER(_lib.Assignment)()
        cands = C.POINTER(_lib.Candidates)()
        check(self.lib.rattle_hip_assign_reads_top(self.h, _ptr(tcat, C.c_uint8) if len(tcat) else None, _ptr(toff, C.c_uint64), len(toff) - 1,
                                                   _ptr(rcat, C.c_uint8) if len(rcat) else None, _ptr(roff, C.c_uint64), len(roff) - 1, k,
                                                   C.byref(P), int(top), C.byref(out), C.byref(cands)))
        self.n = self.k = 0               # the loaded read set was replaced by the last chunk's
        return self._take_assignment(out), self._take_candidates(cands)

    # abundance
    def abundance(self, cands: dict, n_targets: int, ratio=0.95, tol=1e-3, max_iters=1000, iter_block=0) -> dict:
        """Per-target read estimates by the integer fixed-point EM over every read's compatible candidates (rattle_hip_abundance).
        cands: what assign_top returns second, or a hand-built dict with "count" [n], "target" and "score" [n, k].  Slot j of a read is
        compatible iff score[j] >= ratio * score[0].  Returns a dict: units (uint64, 2^-32 read), est_reads, cpm, compatible_reads
        [n_targets]; delta [iterations] (uint64 units); posterior [n, k]; iterations, converged, n_placed.  The same bits on every run,
        whatever iter_block (iterations enqueued between two looks of the host; 0: 32) is."""
        count = np.ascontiguousarray(cands["count"], np.uint32)
        target = np.ascontiguousarray(cands["target"], np.int32)
        score = np.ascontiguousarray(cands["score"], np.float64)
        n, k = target.shape if target.ndim == 2 else (len(count), 0)
        if target.ndim != 2 or score.shape != target.shape or len(count) != n:
            raise ValueError("cands: count [n], target and score [n, k]")
        Cd = _lib.Candidates()
        Cd.n, Cd.k = n, k
        Cd.count = _ptr(count, C.c_uint32); Cd.target = _ptr(target, C.c_int32); Cd.score = _ptr(score, C.c_double)
        P = _lib.AbundanceParams(float(ratio), float(tol), int(max_iters), int(iter_block))
        out = C.POINTER(_lib.Abundance)()
        check(self.lib.rattle_hip_abundance(self.h, C.byref(Cd), int(n_targets), C.byref(P), C.byref(out)))
        R = out.contents
        nt, it = int(R.n_targets), int(R.iterations)

        def arr(ptr, m):
            return np.ctypeslib.as_array(ptr, (max(m, 1),))[:m].copy()

        res = {"units": arr(R.units, nt), "est_reads": arr(R.est_reads, nt), "cpm": arr(R.cpm, nt), "compatible_reads": arr(R.compatible_reads, nt),
               "delta": arr(R.delta, it), "posterior": arr(R.posterior, n * k).reshape(n, k), "iterations": it, "converged": int(R.converged),
               "n_placed": int(R.n_placed)}
        self.lib.rattle_hip_abundance_free(out)
        return res

    @staticmethod
    def _scoring(scoring):
        """(match, mismatch, gap_open, gap_extend), four positive magnitudes, as the library's struct; the library checks the limits"""
        if len(scoring) != 4:
            raise ValueError("scoring is (match, mismatch, gap_open, gap_extend)")
        return _lib.AlignScoring(*(int(v) for v in scoring))

    @staticmethod
    def _align_mode(mode):
        """None for "local" (the four calls without a mode); else the integer the *_mode calls take: 1 for "read", an integer as it is
        (0, RATTLE_ALIGN_LOCAL, goes through the *_mode calls too; the library refuses what it does not know)"""
        if isinstance(mode, str):
            if mode not in ALIGN_MODES:
                raise ValueError('mode is "local" or "read"')
            return None if mode == "local" else ALIGN_MODES[mode]
        return int(mode)

    def align_pairs(self, targets: Sequence[bytes], reads: Sequence[bytes], target_of_read, rev, max_cells=0, pair_chunk=0, scoring=None,
                    mode="local") -> dict:
        """Every read r with target_of_read[r] >= 0 aligned locally to that target, reverse-complemented first where rev[r] == 1
        (rattle_hip_align_pairs, kernel E): the two arrays are `target` and `rev` of an assignment.  Returns a dict of arrays with one
        entry per read (_lib.ALIGN_FIELDS): status (0 aligned, 1 nothing aligns, 2 skipped by max_cells, 3 not submitted), score,
        q_start, q_end (on the read as given), t_start, t_end, matches, mismatches, q_gap, t_gap.
        scoring: None is that call -- match 5, mismatch -4, gap -8 per column; a tuple (match, mismatch, gap_open, gap_extend) of positive
        magnitudes, each in [1, 64] with gap_extend <= gap_open, is rattle_hip_align_pairs_scored: affine gaps, the three-state kernel E,
        also for (5, 4, 8, 8), which gives the records of None.
        mode: "local", or "read" (rattle_hip_align_pairs_mode with RATTLE_ALIGN_READ): the read end to end, the transcript's ends free;
        status 0 for every pair of two non-empty sequences, q_start 0, q_end Lq, a score that may be negative."""
        tcat, toff = pack_reads(targets)
        rcat, roff = pack_reads(reads)
        return self.align_pairs_packed(tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode)

    def align_pairs_packed(self, tcat: np.ndarray, toff: np.ndarray, rcat: np.ndarray, roff: np.ndarray, target_of_read, rev,
                           max_cells=0, pair_chunk=0, scoring=None, mode="local") -> dict:
        """align_pairs() on packed arrays (pack_reads)"""
        return self._align_packed(False, tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode)

    def _align_packed(self, cigar: bool, tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode, pileup=False):
        """The body of align_pairs_packed and (cigar) align_cigars_packed.  mode "local" goes to the calls without a mode -- the plain one
        for scoring None, the _scored one else --, any other mode to the _mode call.  pileup: rattle_hip_align_pileup, the one call
        for every scoring and mode, with or without the CIGARs; returns (records, (offsets, ops) or None, table)."""
        M = self._align_mode(mode)
        P = _lib.AlignParams(int(max_cells), int(pair_chunk))
        n = len(roff) - 1
        t = np.ascontiguousarray(target_of_read, np.int32)
        r = np.ascontiguousarray(rev, np.uint8)
        if len(t) != n or len(r) != n:
            raise ValueError("target_of_read and rev need one entry per read")
        out, cg = C.POINTER(_lib.Alignment)(), C.POINTER(_lib.Cigars)()
        args = (self.h, _ptr(tcat, C.c_uint8) if len(tcat) else None, _ptr(toff, C.c_uint64), len(toff) - 1,
                _ptr(rcat, C.c_uint8) if len(rcat) else None, _ptr(roff, C.c_uint64), n, _ptr(t, C.c_int32) if n else None,
                _ptr(r, C.c_uint8) if n else None, C.byref(P))
        outs = (C.byref(out), C.byref(cg)) if cigar else (C.byref(out),)
        call = "rattle_hip_align_cigars" if cigar else "rattle_hip_align_pairs"
        S = None if scoring is None else self._scoring(scoring)
        pu = C.POINTER(_lib.Pileup)()
        if pileup:
            check(self.lib.rattle_hip_align_pileup(*args, None if S is None else C.byref(S), ALIGN_MODES["local"] if M is None else M,
                                                   C.byref(out), C.byref(cg) if cigar else None, C.byref(pu)))
        elif M is not None:
            check(getattr(self.lib, call + "_mode")(*args, None if S is None else C.byref(S), M, *outs))
        elif S is None:
            check(getattr(self.lib, call)(*args, *outs))
        else:
            check(getattr(self.lib, call + "_scored")(*args, C.byref(S), *outs))
        m = int(out.contents.n)
        res = {f: np.ctypeslib.as_array(getattr(out.contents, f), (max(m, 1),))[:m].copy() for f, _ in _lib.ALIGN_FIELDS}
        self.lib.rattle_hip_alignment_free(out)
        table = None
        if pileup:
            N = int(pu.contents.n)
            table = {f: np.ctypeslib.as_array(getattr(pu.contents, f), (max(N, 1),))[:N].copy() for f in _lib.PILEUP_FIELDS}
            self.lib.rattle_hip_pileup_free(pu)
        if not cigar:
            return (res, None, table) if pileup else res
        offsets = np.ctypeslib.as_array(cg.contents.offset, (m + 1,)).copy()
        total = int(offsets[m])
        ops = np.ctypeslib.as_array(cg.contents.ops, (max(total, 1),))[:total].copy()
        self.lib.rattle_hip_cigars_free(cg)
        return (res, (offsets, ops), table) if pileup else (res, offsets, ops)

    def align_pileup(self, targets: Sequence[bytes], reads: Sequence[bytes], target_of_read, rev, max_cells=0, pair_chunk=0, scoring=None,
                     mode="local", cigars=False):
        """align_cigars(), and what the aligned reads say about every base of every target (rattle_hip_align_pileup, kernels E, F and
        G).  Returns (records, cigars, table): the dict align_pairs returns for the same arguments; (offsets, ops) as align_cigars
        returns them with cigars=True, else None -- the ops then never leave the device --; and a dict of eight uint32 arrays over the
        concatenated targets (_lib.PILEUP_FIELDS; position p is byte p of b"".join(targets)), all on the target's strand: a, c, g, t
        the read bases on '=' and 'X' columns, del the 'D' columns, ins the internal 'I' runs at the base to their right, starts and
        ends the first and last column of every aligned read.  depth is a + c + g + t + del.  scoring and mode: as in align_pairs."""
        tcat, toff = pack_reads(targets)
        rcat, roff = pack_reads(reads)
        return self.align_pileup_packed(tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode, cigars)

    def align_pileup_packed(self, tcat: np.ndarray, toff: np.ndarray, rcat: np.ndarray, roff: np.ndarray, target_of_read, rev,
                            max_cells=0, pair_chunk=0, scoring=None, mode="local", cigars=False):
        """align_pileup() on packed arrays (pack_reads)"""
        return self._align_packed(bool(cigars), tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode, pileup=True)

    def align_cigars(self, targets: Sequence[bytes], reads: Sequence[bytes], target_of_read, rev, max_cells=0, pair_chunk=0, scoring=None,
                     mode="local"):
        """align_pairs(), and the CIGAR of every read that aligns (rattle_hip_align_cigars, kernels E and F).  Returns (records, offsets,
        ops): the dict align_pairs returns for the same arguments, and the ops of read r as ops[offsets[r]:offsets[r + 1]], uint32
        len << 4 | op with BAM's numbers (= 7, X 8, I 1, D 2), from the alignment's start to its end on the strand that was aligned
        (cigar_bytes formats them).  A read whose status is not 0 has none.  scoring: as in align_pairs (a tuple is
        rattle_hip_align_cigars_scored, the three-state kernels E and F).  mode: as in align_pairs ("read" is
        rattle_hip_align_cigars_mode: the ops of a read sum to its whole length, overhangs are I runs at the ends)."""
        tcat, toff = pack_reads(targets)
        rcat, roff = pack_reads(reads)
        return self.align_cigars_packed(tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode)

    def align_cigars_packed(self, tcat: np.ndarray, toff: np.ndarray, rcat: np.ndarray, roff: np.ndarray, target_of_read, rev,
                            max_cells=0, pair_chunk=0, scoring=None, mode="local"):
        """align_cigars() on packed arrays (pack_reads)"""
        return self._align_packed(True, tcat, toff, rcat, roff, target_of_read, rev, max_cells, pair_chunk, scoring, mode)

    def debug_evaluate(self, rects, t_s=0.2, t_v=1000000.0, use_hc=False, is_rna=False, count_pass="auto"):
        """One evaluation of the greedy clustering on the loaded reads (rattle_hip_debug_evaluate, a test hook).
        rects: list of (seed_ids, cand_ids, thr); cand_ids None = triangular (the seeds against each other, pairs s < c).
        count_pass: "auto" (the driver's rule), "seed", "search" or "index".  Returns a dict: "survivors" (with "count"), "kept" and
        "hits", each a dict of arrays rect / seed / cand / strand (indices within the rectangle); "counters" [n_rects, 8];
        "count_pass" (the set of passes that ran); "filter_launches"; "oversize_pairs"; with set_cluster_report on also "evidence":
        arrays bases / hc_bases / variance parallel to "hits", what the verdict kernel's report form wrote for each of them."""
        mode = {"auto": 0, "seed": 1, "search": 2, "index": 3}[count_pass]
        P = ClusterParams(t_s, t_v, 0.0, 0.0, 0.0, 0, int(use_hc), 0.0, int(is_rna))
        keep = []
        R = (_lib.DebugRect * max(len(rects), 1))()
        for r, (seeds, cands, thr) in enumerate(rects):
            s = np.ascontiguousarray(seeds if len(seeds) else [0], np.uint32)
            keep.append(s)
            R[r].seed_ids = _ptr(s, C.c_uint32); R[r].n_seeds = len(seeds); R[r].thr = float(thr)
            if cands is None:
                R[r].triangular = 1
            else:
                c = np.ascontiguousarray(cands if len(cands) else [0], np.uint32)
                keep.append(c)
                R[r].cand_ids = _ptr(c, C.c_uint32); R[r].n_cands = len(cands)
        out = C.POINTER(_lib.DebugEval)()
        check(self.lib.rattle_hip_debug_evaluate(self.h, C.byref(P), mode, R, len(rects), C.byref(out)))
        D = out.contents

        def pairs(Q, with_count):
            n = Q.n
            d = {f: np.ctypeslib.as_array(getattr(Q, f), (max(n, 1),))[:n].copy() for f in ("rect", "seed", "cand", "strand")}
            if with_count:
                d["count"] = np.ctypeslib.as_array(Q.count, (max(n, 1),))[:n].copy()
            return d

        res = {"survivors": pairs(D.survivors, True), "kept": pairs(D.kept, False), "hits": pairs(D.hits, False),
               "counters": np.ctypeslib.as_array(D.counters, (len(rects) * 8 + 1,))[:len(rects) * 8].reshape(len(rects), 8).copy(),
               "count_pass": {p for b, p in ((1, "seed"), (2, "search"), (4, "index")) if D.count_pass & b},
               "filter_launches": int(D.filter_launches), "oversize_pairs": int(D.oversize_pairs)}
        if D.hit_bases:
            nh = D.hits.n
            res["evidence"] = {f: np.ctypeslib.as_array(getattr(D, "hit_" + f), (max(nh, 1),))[:nh].copy() for f in ("bases", "hc_bases", "variance")}
        self.lib.rattle_hip_debug_evaluate_free(out)
        return res

    def debug_post_msa(self, packs, mode: int, min_occ=0.3, gap_occ=0.3, err_ratio=30.0, vote_order: bytes = b""):
        """Kernel D alone on given MSAs (rattle_hip_debug_post_msa, a test hook), all packs in one launch.  packs: a list of
        (width, sequences, columns per sequence, qualities per sequence or None), see msa_pack.  Returns a list with one dict per
        pack: moff, coff, rfirst, rlast, cons (bytes, one per column); mode 1: tfront, tback, olen, reads [(seq, qual)], flag, sym,
        err (float64; .view(uint64) for the bits) and, with set_correction_report on, the six per-row counters match, substituted,
        mismatch_kept, inserted, deleted, gap_kept; mode 2: consensus (bytes)."""
        first = np.zeros(len(packs) + 1, np.uint32)
        first[1:] = np.cumsum([len(p[1]) for p in packs])
        width = np.array([p[0] for p in packs] + [0], np.uint32)
        seqs = [s for p in packs for s in p[1]]
        cat, off = pack_reads(seqs)
        col = np.concatenate([np.asarray(c, np.uint32) for p in packs for c in p[2]] + [np.zeros(1, np.uint32)])
        assert len(col) == len(cat) + 1, "one column per base"
        have_q = [p[3] is not None for p in packs]
        qcat = None
        if any(have_q):
            assert all(have_q), "qualities for every pack or for none"
            qcat, qoff = pack_reads([q for p in packs for q in p[3]])
            assert np.array_equal(off, qoff), "sequence and quality lengths differ"
        M = _lib.DebugMsa(len(packs), _ptr(first, C.c_uint32), _ptr(width, C.c_uint32), _ptr(off, C.c_uint64),
                          _ptr(cat, C.c_uint8) if len(cat) else None, _ptr(qcat, C.c_uint8) if qcat is not None and len(qcat) else None,
                          _ptr(col, C.c_uint32))
        P, _ = correct_params(min_occ, gap_occ, err_ratio, vote_order=vote_order)
        out = C.POINTER(_lib.DebugPost)()
        check(self.lib.rattle_hip_debug_post_msa(self.h, C.byref(P), mode, C.byref(M), C.byref(out)))
        D = out.contents

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, (max(int(n), 1),))[:int(n)].copy()

        n, ncol, npk = D.n_rows, D.n_cols, D.n_packs
        moff, coff = arr(D.moff, npk), arr(D.coff, npk)
        rfirst, rlast, cons = arr(D.rfirst, n), arr(D.rlast, n), arr(D.cons, ncol)
        if mode == 1:
            tfront, tback, olen, ooff = arr(D.tfront, n), arr(D.tback, n), arr(D.olen, n), arr(D.out_off, n + 1)
            oseq, oqual = arr(D.out_seq, ooff[n]).tobytes(), arr(D.out_qual, ooff[n]).tobytes()
            flag, sym, err = arr(D.flag, ncol), arr(D.sym, ncol), arr(D.err, ncol)
            counters = {f: arr(getattr(D, f), n) for f in _lib.REPORT_COUNTERS if getattr(D, f)}
        else:
            clen, consensus = arr(D.cons_len, npk), arr(D.consensus, ncol)
        self.lib.rattle_hip_debug_post_msa_free(out)
        res = []
        for p in range(npk):
            a, b = int(first[p]), int(first[p + 1])
            c0, c1 = int(coff[p]), int(coff[p]) + int(width[p])
            d = {"moff": int(moff[p]), "coff": c0, "rfirst": rfirst[a:b], "rlast": rlast[a:b], "cons": cons[c0:c1].tobytes()}
            if mode == 1:
                d.update(tfront=tfront[a:b], tback=tback[a:b], olen=olen[a:b], flag=flag[c0:c1], sym=sym[c0:c1], err=err[c0:c1],
                         reads=[(oseq[int(ooff[q]):int(ooff[q + 1])], oqual[int(ooff[q]):int(ooff[q + 1])]) for q in range(a, b)])
                d.update({f: v[a:b] for f, v in counters.items()})
            else:
                d["consensus"] = consensus[c0:c0 + int(clen[p])].tobytes()
            res.append(d)
        return res

    def debug_consensus_support(self, packs, sup=None, dep=None, vote_order: bytes = b""):
        """The mode-2 report form of kernel D alone on given MSAs (rattle_hip_debug_consensus_support, a test hook), all packs in one
        launch.  packs as for debug_post_msa (qualities ignored); sup / dep: per pack, per row, a uint32 array with one value per base
        (both None: rows that are reads, level 2).  Returns one dict per pack: consensus (bytes) and support, depth, pack_support,
        pack_depth (uint32 per base of the consensus; None where the hook returns NULL: all four with set_consensus_support off,
        the pack_* pair at level 2)."""
        first = np.zeros(len(packs) + 1, np.uint32)
        first[1:] = np.cumsum([len(p[1]) for p in packs])
        width = np.array([p[0] for p in packs] + [0], np.uint32)
        cat, off = pack_reads([s for p in packs for s in p[1]])
        col = np.concatenate([np.asarray(c, np.uint32) for p in packs for c in p[2]] + [np.zeros(1, np.uint32)])
        assert len(col) == len(cat) + 1, "one column per base"
        assert (sup is None) == (dep is None)
        vals = []
        for v in (sup, dep):
            if v is not None:
                v = np.concatenate([np.asarray(r, np.uint32) for p in v for r in p] + [np.zeros(1, np.uint32)])
                assert len(v) == len(cat) + 1, "one support and one depth per base"
            vals.append(v)
        M = _lib.DebugSupportMsa(len(packs), _ptr(first, C.c_uint32), _ptr(width, C.c_uint32), _ptr(off, C.c_uint64),
                                 _ptr(cat, C.c_uint8) if len(cat) else None, _ptr(col, C.c_uint32),
                                 None if vals[0] is None else _ptr(vals[0], C.c_uint32), None if vals[1] is None else _ptr(vals[1], C.c_uint32))
        P, _ = correct_params(vote_order=vote_order)
        out = C.POINTER(_lib.DebugSupport)()
        check(self.lib.rattle_hip_debug_consensus_support(self.h, C.byref(P), C.byref(M), C.byref(out)))
        D = out.contents
        npk, ncol = D.n_packs, int(D.n_cols)

        def arr(ptr, n):
            return np.ctypeslib.as_array(ptr, (max(int(n), 1),))[:int(n)].copy() if ptr else None

        coff, clen, cons = arr(D.coff, npk), arr(D.cons_len, npk), arr(D.consensus, ncol)
        fields = {f: arr(getattr(D, f), ncol) for f in _lib.SUPPORT_FIELDS}
        level = D.level
        self.lib.rattle_hip_debug_consensus_support_free(out)
        res = []
        for p in range(npk):
            a, b = int(coff[p]), int(coff[p]) + int(clen[p])
            d = {"level": level, "consensus": cons[a:b].tobytes()}
            d.update({f: None if v is None else v[a:b] for f, v in fields.items()})
            res.append(d)
        return res

    def kernel_stats(self, kernel: int):
        ms = C.c_double(); n = C.c_uint64(); b = C.c_uint64()
        check(self.lib.rattle_hip_kernel_stats(self.h, kernel, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def reset_stats(self):
        check(self.lib.rattle_hip_kernel_stats_reset(self.h))

    def stage_ms(self, reset: bool = True):
        """Host wall time of `correct`'s stages since the last reset: {stage: ms} (rattle_hip_stage_ms)."""
        ms = (C.c_double * 8)()
        check(self.lib.rattle_hip_stage_ms(self.h, ms, 1 if reset else 0))
        return {"1": ms[1], "2a": ms[2], "2b+3a": ms[3], "3b": ms[4]}


def min_common_lut(thr: float) -> np.ndarray:
    """min_common_lut[m] = smallest c with float(c)/float(m) >= thr (cluster.cpp:19,43); 0xFFFF = never."""
    lut = np.full(4097, 0xFFFF, np.uint16)
    for m in range(1, 4097):
        c = np.arange(0, 4097, dtype=np.float64) / float(m)
        idx = np.nonzero(c >= thr)[0]
        if len(idx):
            lut[m] = idx[0]
    return lut


def cluster_command(ctx: Context, seqs: Sequence[bytes], ann: Sequence[int], *, k=10, t_s=0.2, t_v=1000000.0,
                    iso=False, iso_k=11, iso_t_s=0.3, iso_t_v=25.0, bv_threshold=0.4, bv_min_threshold=0.2,
                    bv_falloff=0.05, repr_percentile=0.15, is_rna=False, report=False):
    """`rattle cluster` after input parsing (main.cpp:254-323).  `seqs`/`ann` are the filtered reads
    and their original record indices.  Returns clusters in rattle_amd.hps list form and the counters; report=True: also the
    cluster report (Clusters.report(): gene-level joins, then with iso the level-1 joins of every gene in gene order; into / absorbed
    are record indices), made with the context's switch on for the length of the call."""
    if report:
        was = ctx.cluster_report
        ctx.set_cluster_report(True)
        try:
            return _cluster_command(ctx, seqs, ann, k, t_s, t_v, iso, iso_k, iso_t_s, iso_t_v, bv_threshold, bv_min_threshold, bv_falloff,
                                    repr_percentile, is_rna, True)
        finally:
            ctx.set_cluster_report(was)
    return _cluster_command(ctx, seqs, ann, k, t_s, t_v, iso, iso_k, iso_t_s, iso_t_v, bv_threshold, bv_min_threshold, bv_falloff,
                            repr_percentile, is_rna, False)


def _cluster_command(ctx, seqs, ann, k, t_s, t_v, iso, iso_k, iso_t_s, iso_t_v, bv_threshold, bv_min_threshold, bv_falloff,
                     repr_percentile, is_rna, report):
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))       # stable, length desc (fasta.cpp:462)
    sseqs = [seqs[i] for i in order]
    sann = [ann[i] for i in order]
    ann_of = np.asarray(sann, np.int64)

    def joins_of(cl, ids, level):
        """a set's joins with its ids (positions in `ids`) as record indices"""
        j = dict(cl.report())
        j["into"] = ann_of[ids[j["into"]]].astype(np.int32); j["absorbed"] = ann_of[ids[j["absorbed"]]].astype(np.int32)
        j["level"] = np.full(len(j["into"]), level, np.uint8)
        return j

    ctx.load_reads(sseqs, k, not is_rna)
    gene = ctx.cluster_reads(t_s, t_v, bv_threshold, bv_min_threshold, bv_falloff, 0, False, repr_percentile, is_rna)
    gl = gene.as_list()
    parts = [joins_of(gene, np.arange(len(sseqs)), 0)] if report else []
    if not iso:
        res = [((sann[m[0]], m[1], -1), [(sann[s[0]], s[1], -1) for s in mem]) for m, mem in gl], gene.counters
        return res + (concat_reports(parts),) if report else res
    ctx.load_reads(sseqs, iso_k, not is_rna)
    out = []
    counters = gene.counters.copy()
    subsets = []
    for m, mem in gl:
        ids = [s[0] for s in mem]
        ids.sort(key=lambda x: -x)                                       # main.cpp:285-291
        ids.sort(key=lambda x: -len(sseqs[x]))
        subsets.append(np.array(ids, np.uint32))
    subs = ctx.cluster_subsets(subsets, iso_t_s, iso_t_v, bv_threshold, bv_min_threshold, bv_falloff, repr_percentile, is_rna)
    for gi, (ids, sub) in enumerate(zip(subsets, subs)):
        counters += sub.counters
        for im, imem in sub.as_list():
            out.append(((sann[int(ids[im[0]])], im[1], gi), [(sann[int(ids[s[0]])], s[1], gi) for s in imem]))
        if report:
            parts.append(joins_of(sub, ids.astype(np.int64), 1))
    return (out, counters, concat_reports(parts)) if report else (out, counters)


def correct_command(ctx: Context, headers: Sequence[bytes], seqs: Sequence[bytes], quals: Sequence[bytes], clusters, *,
                    min_occ=0.3, gap_occ=0.3, split=200, min_reads=5, n_threads=0, vote_order=b"", pack_order=None,
                    ann: Optional[Sequence[bytes]] = None, max_pack_cells=0, gather_root: Optional[int] = None,
                    with_skipped=False, support=False):
    """`rattle correct` after input parsing (main.cpp:396-408): returns the three FASTQ texts
    (corrected, uncorrected, consensi) with the headers correct.cpp:348-353,540-549 builds
    (no -l labels: `labels=` is empty).  `ann` = the third line of each input record: uncorrected reads
    keep theirs (the reference pushes the original read_t, correct.cpp:362-366,289-293); corrected reads
    and consensi get "+" (:286, :469).  support=True: the call runs with the context's consensus support on (one device) and the
    text of consensus_support.tsv (support_tsv) is appended to the result."""
    was = ctx.consensus_support
    if support:
        ctx.set_consensus_support(True)
    try:
        res = ctx.correct_reads(seqs, quals, clusters, min_occ, gap_occ, 30.0, split, min_reads, n_threads, vote_order, pack_order,
                                max_pack_cells, gather_root)
    finally:
        if support:
            ctx.set_consensus_support(was)
    if res is None:
        return None
    gene_mode = len(clusters) == 0 or clusters[0][0][2] == -1

    def tag(cid):
        gid = clusters[cid][0][2]
        if gid == -1:
            return b",gene_cluster_%d" % cid
        return b",gene_cluster_%d,transcript_cluster_%d" % (gid, cid)

    def fq(recs, keep_ann):
        return b"".join(b"%s%s\n%s\n%s\n%s\n" % (headers[r[0]], tag(r[1]), r[3], ann[r[0]] if keep_ann and ann is not None else b"+", r[4])
                        for r in recs)

    cons = []
    for rid, cid, nr, s, q in res["consensi"]:
        if gene_mode:
            h = b"@gene_cluster_%d reads=%d labels=" % (cid, nr)
        else:
            h = b"@transcript_cluster_%d gene_cluster_%d reads=%d labels=" % (cid, clusters[cid][0][2], nr)
        cons.append(b"%s\n%s\n+\n%s\n" % (h, s, q))
    out = (fq(res["corrected"], False), fq(res["uncorrected"], True), b"".join(cons), res["counters"])
    if with_skipped:
        out = out + (res["skipped"],)
    if support:
        names = [(b"gene_cluster_%d" if gene_mode else b"transcript_cluster_%d") % r[1] for r in res["consensi"]]
        out = out + (support_tsv(names, [r[2] for r in res["consensi"]], res["support"]),)
    return out


def _first_token(header: bytes) -> bytes:
    """the id of a record: the first token of its header, without its '@' / '>'"""
    h = (header[1:] if header[:1] in (b"@", b">") else header).lstrip(b" \t")
    return h.replace(b"\t", b" ").split(b" ", 1)[0]


def unassigned_records(n: int) -> dict:
    """n records of assign as the library makes them for reads that nothing accepts"""
    rec = {f: np.zeros(n, np.dtype(t)) for f, t in _lib.ASSIGN_FIELDS}
    rec["target"][:] = -1
    rec["score"][:] = -1.0
    rec["second_score"][:] = -1.0
    return rec


def assignments_tsv(read_names: Sequence[bytes], target_names: Sequence[bytes], rec: dict) -> bytes:
    """assignments.tsv as `rattle assign` writes it: a header line, then one line per read in file order: read, target ('*':
    unassigned), strand (+ / - / *), score, second_score, n_accepted, bases, hc_bases, min_len, variance; doubles as %.17g."""
    lines = [b"read\ttarget\tstrand\tscore\tsecond_score\tn_accepted\tbases\thc_bases\tmin_len\tvariance\n"]
    for i, name in enumerate(read_names):
        t = int(rec["target"][i])
        lines.append(b"%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
            name, target_names[t] if t >= 0 else b"*", b"*" if t < 0 else b"-" if rec["rev"][i] else b"+",
            ("%.17g" % rec["score"][i]).encode(), ("%.17g" % rec["second_score"][i]).encode(), int(rec["n_accepted"][i]),
            int(rec["bases"][i]), int(rec["hc_bases"][i]), int(rec["min_len"][i]), ("%.17g" % rec["variance"][i]).encode()))
    return b"".join(lines)


def target_counts_tsv(target_names: Sequence[bytes], target_lengths: Sequence[int], rec: dict) -> bytes:
    """target_counts.tsv: a header line, then one line per target in file order: target, length, reads (the reads whose best is this
    target), unique_reads (those among them that no other target accepts: second_score < 0)."""
    t = np.asarray(rec["target"], np.int64)
    hit = t >= 0
    reads = np.bincount(t[hit], minlength=len(target_names))
    uniq = np.bincount(t[hit & (np.asarray(rec["second_score"]) < 0)], minlength=len(target_names))
    return b"target\tlength\treads\tunique_reads\n" + b"".join(
        b"%s\t%d\t%d\t%d\n" % (n, int(l), int(reads[i]), int(uniq[i])) for i, (n, l) in enumerate(zip(target_names, target_lengths)))


def abundance_tsv(target_names: Sequence[bytes], target_lengths: Sequence[int], rec: dict, ab: dict) -> bytes:
    """abundance.tsv as `rattle assign --abundance` writes it: a header line, then one line per target in file order: target, length,
    reads and unique_reads (the columns of target_counts.tsv), compatible_reads, est_reads, cpm (Context.abundance); doubles as %.17g."""
    t = np.asarray(rec["target"], np.int64)
    hit = t >= 0
    reads = np.bincount(t[hit], minlength=len(target_names))
    uniq = np.bincount(t[hit & (np.asarray(rec["second_score"]) < 0)], minlength=len(target_names))
    return b"target\tlength\treads\tunique_reads\tcompatible_reads\test_reads\tcpm\n" + b"".join(
        b"%s\t%d\t%d\t%d\t%d\t%s\t%s\n" % (n, int(l), int(reads[i]), int(uniq[i]), int(ab["compatible_reads"][i]),
                                        ("%.17g" % ab["est_reads"][i]).encode(), ("%.17g" % ab["cpm"][i]).encode())
        for i, (n, l) in enumerate(zip(target_names, target_lengths)))


def _abundance_text(ctx, target_headers, targets, rec, cands8, abundance):
    """abundance = (ratio, tol, max_iters): the EM over the 8-slot list of all reads, as the bytes of abundance.tsv"""
    ab = ctx.abundance(cands8, len(targets), *abundance)
    return abundance_tsv([_first_token(h) for h in target_headers], [len(s) for s in targets], rec, ab)


def _assign_submitted(ctx, reads, targets, k, t_s, t_v, bv_threshold, is_rna, count_pass, target_batch, read_chunk, secondary, abundance=False):
    """the clean reads through assign (secondary == 0) or assign_top, spread back over all reads: (record, candidates or None, None).
    abundance: the list is made with 8 slots whatever secondary is and comes third; the second is its first secondary + 1 slots (the
    list has the prefix property: they are what the shorter list holds), None without secondary."""
    if not 0 <= int(secondary) <= 7:
        raise ValueError("secondary is in 0..7")
    sent = [i for i, s in enumerate(reads) if not s.translate(None, b"ACGTU")]
    rec = unassigned_records(len(reads))
    cands = None
    top = 8 if abundance else secondary + 1
    if secondary or abundance:
        got, part = ctx.assign_top(targets, [reads[i] for i in sent], top, k, t_s, t_v, bv_threshold, False, is_rna, target_batch,
                                   read_chunk, count_pass)
        cands = unused_candidates(len(reads), top)
        for f in cands:
            cands[f][sent] = part[f]
    else:
        got = ctx.assign(targets, [reads[i] for i in sent], k, t_s, t_v, bv_threshold, False, is_rna, target_batch, read_chunk, count_pass)
    for f in rec:
        rec[f][sent] = got[f]
    if not abundance:
        return rec, cands, None
    first = None
    if secondary:
        first = {f: np.ascontiguousarray(v[:, :secondary + 1]) for f, v in cands.items() if f != "count"}
        first["count"] = np.minimum(cands["count"], secondary + 1).astype(np.uint32)
    return rec, first, cands


def unused_candidates(n: int, top: int) -> dict:
    """the candidate lists of n reads that nothing accepts, as the library makes them"""
    c = {f: np.zeros((n, top), np.dtype(t)) for f, t in _lib.CANDIDATE_FIELDS}
    c["count"] = np.zeros(n, np.uint32)
    c["target"][:] = -1
    c["score"][:] = -1.0
    return c


def candidates_tsv(read_names: Sequence[bytes], target_names: Sequence[bytes], cands: dict) -> bytes:
    """candidates.tsv as `rattle assign --secondary N` writes it: a header line, then one line per filled slot, in file order of the
    reads and then by rank: read, rank (0-based), target, strand (+ / -), score, bases, hc_bases, min_len, variance; doubles as
    %.17g.  A read with no candidate has no line."""
    lines = [b"read\trank\ttarget\tstrand\tscore\tbases\thc_bases\tmin_len\tvariance\n"]
    for i, name in enumerate(read_names):
        for j in range(int(cands["count"][i])):
            lines.append(b"%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%s\n" % (
                name, j, target_names[int(cands["target"][i, j])], b"-" if cands["rev"][i, j] else b"+",
                ("%.17g" % cands["score"][i, j]).encode(), int(cands["bases"][i, j]), int(cands["hc_bases"][i, j]),
                int(cands["min_len"][i, j]), ("%.17g" % cands["variance"][i, j]).encode()))
    return b"".join(lines)


def assign_command(ctx: Context, read_headers: Sequence[bytes], reads: Sequence[bytes], target_headers: Sequence[bytes],
                   targets: Sequence[bytes], *, k=10, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, is_rna=False, count_pass="auto",
                   target_batch=0, read_chunk=0, secondary=0, abundance=False, abundance_ratio=0.95, abundance_tol=1e-3, abundance_iters=1000):
    """`rattle assign -i reads -x transcripts` after input parsing: every record of both files takes part, in file order.  Returns the
    bytes of assignments.tsv and of target_counts.tsv.  A read with a base other than A, C, G, T, U is not compared: unassigned.
    secondary=N (1..7) is `--secondary N`: the first two are unchanged and the bytes of candidates.tsv (candidates_tsv, N + 1 slots per
    read) come third.  abundance=True is `--abundance`: the candidate list is made with 8 slots whatever secondary is, the files above
    do not change, and the bytes of abundance.tsv (abundance_tsv; Context.abundance with abundance_ratio, abundance_tol, abundance_iters)
    come last."""
    rec, cands, all8 = _assign_submitted(ctx, reads, targets, k, t_s, t_v, bv_threshold, is_rna, count_pass, target_batch, read_chunk, secondary,
                                          abundance)
    tn = [_first_token(h) for h in target_headers]
    rn = [_first_token(h) for h in read_headers]
    out = (assignments_tsv(rn, tn, rec), target_counts_tsv(tn, [len(s) for s in targets], rec))
    if cands is not None:
        out = out + (candidates_tsv(rn, tn, cands),)
    if abundance:
        out = out + (_abundance_text(ctx, target_headers, targets, rec, all8, (abundance_ratio, abundance_tol, abundance_iters)),)
    return out


_CIGAR_LETTER = {1: b"I", 2: b"D", 7: b"=", 8: b"X"}


def cigar_bytes(ops) -> bytes:
    """the ops of one read (align_cigars: len << 4 | op) as a CIGAR string, b"12=1X3I...": the extended set, no clipping op"""
    return b"".join(b"%d%s" % (int(o) >> 4, _CIGAR_LETTER[int(o) & 15]) for o in ops)


def _paf_line(name, lq, tname, lt, rev, alignment, i, tags=b"") -> bytes:
    """the PAF line of entry i of an alignment record set, up to and including nd:i:, then `tags`; no line end"""
    M, X, qg, tg = (int(alignment[f][i]) for f in ("matches", "mismatches", "q_gap", "t_gap"))
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tAS:i:%d\tNM:i:%d\tnx:i:%d\tni:i:%d\tnd:i:%d%s" % (
        name, int(lq), int(alignment["q_start"][i]), int(alignment["q_end"][i]), b"-" if rev else b"+", tname, int(lt),
        int(alignment["t_start"][i]), int(alignment["t_end"][i]), M, M + X + qg + tg, int(alignment["score"][i]), X + qg + tg, X, qg, tg, tags)


def _cigar_tag(cigars, i) -> bytes:
    return b"" if cigars is None else b"\tcg:Z:" + cigar_bytes(cigars[1][int(cigars[0][i]):int(cigars[0][i + 1])])


def paf_text(read_names: Sequence[bytes], read_lengths: Sequence[int], target_names: Sequence[bytes], target_lengths: Sequence[int],
             assignment: dict, alignment: dict, cigars=None) -> bytes:
    """alignments.paf as `rattle assign --paf` writes it: one line per read with status 0, in file order (none for unassigned, unaligned
    or skipped reads): read, Lq, q_start, q_end, + / -, target, Lt, t_start, t_end, matches, columns (matches + mismatches + q_gap +
    t_gap), 255, AS:i:score, NM:i:mismatches + q_gap + t_gap, nx:i:mismatches, ni:i:q_gap, nd:i:t_gap.  cigars: (offsets, ops) of
    align_cigars; with them every line ends in a further tag, cg:Z:<the read's CIGAR> (`--paf --cigar`)."""
    lines = []
    for i in np.nonzero(np.asarray(alignment["status"]) == 0)[0]:
        t = int(assignment["target"][i])
        lines.append(_paf_line(read_names[i], read_lengths[i], target_names[t], target_lengths[t], assignment["rev"][i], alignment, i,
                               _cigar_tag(cigars, i)) + b"\n")
    return b"".join(lines)


def paf_ranked_text(read_names: Sequence[bytes], read_lengths: Sequence[int], target_names: Sequence[bytes], target_lengths: Sequence[int],
                    cands: dict, alignments: Sequence[dict], cigars=None) -> bytes:
    """alignments.paf as `rattle assign --paf --secondary N` writes it.  alignments[j] is the alignment record set of rank j: every
    read on its slot j (align_ranks); ranks beyond len(alignments) have no line.  One line per (read, rank) whose own alignment has
    status 0, in file order of the reads and then by rank; the fields of paf_text, then tp:A:P (rank 0) or tp:A:S and rk:i:<rank>
    behind nd:i: and, with cigars (one (offsets, ops) per rank), before cg:Z:."""
    lines = []
    ok = [np.asarray(a["status"]) == 0 for a in alignments]
    for i, name in enumerate(read_names):
        for j in range(min(int(cands["count"][i]), len(alignments))):
            if not ok[j][i]:
                continue
            t = int(cands["target"][i, j])
            tags = (b"\ttp:A:P" if j == 0 else b"\ttp:A:S") + b"\trk:i:%d" % j + _cigar_tag(None if cigars is None else cigars[j], i)
            lines.append(_paf_line(name, read_lengths[i], target_names[t], target_lengths[t], cands["rev"][i, j], alignments[j], i, tags) + b"\n")
    return b"".join(lines)


def pileup_tsv(target_names: Sequence[bytes], targets: Sequence[bytes], pileup: dict) -> bytes:
    """pileup.tsv as `rattle assign --paf --pileup` writes it: a header, then one line per transcript position with depth > 0, in file
    order: target, pos (0-based), ref (the transcript's byte as given), depth (A + C + G + T + del), A, C, G, T, del, ins, starts,
    ends.  pileup: the table of Context.align_pileup over these targets.  A position of depth 0 has no line and no count."""
    lines = [b"target\tpos\tref\tdepth\tA\tC\tG\tT\tdel\tins\tstarts\tends\n"]
    planes = [np.asarray(pileup[f], np.int64) for f in _lib.PILEUP_FIELDS]
    depth = planes[0] + planes[1] + planes[2] + planes[3] + planes[4]
    base = 0
    for name, s in zip(target_names, targets):
        for pos in np.nonzero(depth[base:base + len(s)])[0]:
            p = base + int(pos)
            lines.append(b"%s\t%d\t%s\t%d\t%s\n" % (name, pos, s[pos:pos + 1], depth[p], b"\t".join(b"%d" % int(pl[p]) for pl in planes)))
        base += len(s)
    return b"".join(lines)


def align_ranks(ctx: Context, targets: Sequence[bytes], reads: Sequence[bytes], cands: dict, max_cells=0, pair_chunk=0, cigar=False,
                scoring=None, mode="local", pileup=False):
    """Every read aligned to each of its candidates: one call of Context.align_pairs (cigar: align_cigars) per rank j, with slot j's
    target and strand as target_of_read and rev, up to the first rank no read has, every rank in the same `mode`.  Returns
    (alignments, cigars): one record set per rank, and one (offsets, ops) per rank or None.  pileup=True: rank 0's call is
    Context.align_pileup, which returns the same records and CIGARs, and its table comes third (None if no read has a candidate)."""
    alns, cgs, table = [], [], None
    for j in range(cands["target"].shape[1]):
        if not (np.asarray(cands["count"]) > j).any():
            break
        t = np.ascontiguousarray(cands["target"][:, j]); r = np.ascontiguousarray(cands["rev"][:, j])
        if pileup and j == 0:
            aln, cg, table = ctx.align_pileup(targets, reads, t, r, max_cells, pair_chunk, scoring, mode, cigars=cigar)
            if cigar:
                cgs.append(cg)
        elif cigar:
            aln, offsets, ops = ctx.align_cigars(targets, reads, t, r, max_cells, pair_chunk, scoring, mode)
            cgs.append((offsets, ops))
        else:
            aln = ctx.align_pairs(targets, reads, t, r, max_cells, pair_chunk, scoring, mode)
        alns.append(aln)
    return (alns, (cgs if cigar else None), table) if pileup else (alns, (cgs if cigar else None))


def assign_paf_command(ctx: Context, read_headers: Sequence[bytes], reads: Sequence[bytes], target_headers: Sequence[bytes],
                       targets: Sequence[bytes], *, k=10, t_s=0.2, t_v=1000000.0, bv_threshold=0.4, is_rna=False, count_pass="auto",
                       target_batch=0, read_chunk=0, max_cells=0, pair_chunk=0, cigar=False, scoring=None, secondary=0,
                       end_to_end=False, abundance=False, abundance_ratio=0.95, abundance_tol=1e-3, abundance_iters=1000, pileup=False):
    """`rattle assign --paf`: assign_command, then every placed read aligned to its transcript (Context.align_pairs).  Returns the bytes
    of assignments.tsv, target_counts.tsv and alignments.paf; the first two are what assign_command returns.  cigar=True is
    `--paf --cigar`: Context.align_cigars, and a cg:Z: tag on every line.  scoring=(m, x, o, e) is `--paf-scoring m,x,o,e`: affine gaps
    (Context.align_pairs); None is the linear default.  secondary=N (1..7) is `--secondary N`: every read is aligned to each of its
    N + 1 candidates (align_ranks), alignments.paf is the ranked one (paf_ranked_text) and the bytes of candidates.tsv come fourth.
    end_to_end=True is `--paf-end-to-end`: every alignment, of every rank, in mode "read" -- the whole read on every line; the tables
    do not change.  abundance=True is `--abundance`, as for assign_command: the bytes of abundance.tsv come last, nothing else changes.
    pileup=True is `--pileup`: the alignment of every read on its transcript (rank 0 under `secondary`) is Context.align_pileup, with or
    without `cigar`, and the bytes of pileup.tsv (pileup_tsv) come behind everything else; the other bytes do not change."""
    mode = "read" if end_to_end else "local"
    rec, cands, all8 = _assign_submitted(ctx, reads, targets, k, t_s, t_v, bv_threshold, is_rna, count_pass, target_batch, read_chunk, secondary,
                                          abundance)
    last = ()
    if abundance:
        last = (_abundance_text(ctx, target_headers, targets, rec, all8, (abundance_ratio, abundance_tol, abundance_iters)),)
    tn = [_first_token(h) for h in target_headers]
    rn = [_first_token(h) for h in read_headers]
    tl = [len(s) for s in targets]
    rl = [len(s) for s in reads]
    if cands is not None:
        alns, cgs, *table = align_ranks(ctx, targets, reads, cands, max_cells, pair_chunk, cigar, scoring, mode, pileup)
        if pileup:
            if table[0] is None:                # no read has a candidate: nothing was aligned
                table = [{f: np.zeros(sum(tl), np.uint32) for f in _lib.PILEUP_FIELDS}]
            last += (pileup_tsv(tn, targets, table[0]),)
        return (assignments_tsv(rn, tn, rec), target_counts_tsv(tn, tl, rec), paf_ranked_text(rn, rl, tn, tl, cands, alns, cgs),
                candidates_tsv(rn, tn, cands)) + last
    cigars = None
    if pileup:
        aln, cigars, table = ctx.align_pileup(targets, reads, rec["target"], rec["rev"], max_cells, pair_chunk, scoring, mode, cigars=cigar)
        last += (pileup_tsv(tn, targets, table),)
    elif cigar:
        aln, offsets, ops = ctx.align_cigars(targets, reads, rec["target"], rec["rev"], max_cells, pair_chunk, scoring, mode)
        cigars = (offsets, ops)
    else:
        aln = ctx.align_pairs(targets, reads, rec["target"], rec["rev"], max_cells, pair_chunk, scoring, mode)
    return (assignments_tsv(rn, tn, rec), target_counts_tsv(tn, tl, rec), paf_text(rn, rl, tn, tl, rec, aln, cigars)) + last
