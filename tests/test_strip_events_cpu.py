"""CPU: the construction of tests/test_gpu_strip_events.py's Z-drop pairs, checked on the oracle alone: among the oracle's own
records there is a dropped pair whose drop row falls in each place a strip can have in a (64, 16) fill (first, middle and last strip
of a round of 64, the last incomplete round, a strip that takes the row-by-row epilogue), and there are pairs that do not drop, with
and without a Z-drop set.  A guard for that test's inputs; no kernel code runs here."""
from oracle import pyoracle as po
from tests import parity_util as pu
from tests import test_gpu_strip_events as se


def test_drop_rows_cover_every_class():
    qs, ts, ws, zs, cls = se.batch()
    exp = pu.oracle_batch(False, qs, ts, se.MAT, se.GQ, se.GE, 0, 0, ws, zs, 0, po.SCORE_ONLY)
    seen = {c: 0 for c in se.CLASSES}
    for i, c in enumerate(cls):
        if c is not None:
            assert exp[i]["zdropped"] == 1, i
            seen[c] += 1
    print("drop rows per class:", seen)
    assert all(seen[c] > 0 for c in se.CLASSES), seen
    assert sum(1 for i, r in enumerate(exp) if zs[i] < 0 and r["zdropped"] == 0) > 0
    assert sum(1 for i, r in enumerate(exp) if zs[i] >= 0 and r["zdropped"] == 0) > 0
