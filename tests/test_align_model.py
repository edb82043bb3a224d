"""tests/align_model.py against answers on record: tests/golden/align_pairs_ref.json.gz holds the record and the CIGAR of every distinct
(read, transcript, strand, scoring, mode) the cases of align_affine_ref and align_ends_ref submit, as those two modules gave them when
each had its own copy of the recurrence (tools/record_align_ref.py).  The model has to give every one of them again, exactly, in both of
its forms, and kernel F's form has to give the ops from the record alone.  No device."""
import os
import sys

import align_model as M
import align_ref as R
import cigar_ref as CG

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_align_ref as REC  # noqa: E402

GOLDEN = REC.load()
TODAY = REC.submissions()


def test_the_fixture_holds_todays_pairs_and_no_other():
    assert not TODAY.keys() - GOLDEN.keys(), "the cases submit pairs that are not on record: run tools/record_align_ref.py"
    assert not GOLDEN.keys() - TODAY.keys(), "pairs on record that no case submits"


def test_the_model_gives_every_recorded_answer_in_all_three_forms():
    checked = 0
    for k, (q, t, s, sc, mode, _) in TODAY.items():
        rec, cigar = GOLDEN[k]
        got, ops = M.pair(q, t, s, sc, mode)
        assert (got, CG.text(ops)) == (rec, cigar), (q, t, s, sc, mode)
        assert M.pair(q, t, s, sc, mode, "forward")[0] == rec, (q, t, s, sc, mode)
        if rec[0] == 0:
            on_strand = rec[:2] + (len(q) - rec[3], len(q) - rec[2]) + rec[4:] if s else rec
            assert M.rectangle(R.revcomp(q) if s else q, t, on_strand, sc, mode)[0] == ops, (q, t, s, sc, mode)
        checked += 1
    assert checked == len(GOLDEN)
