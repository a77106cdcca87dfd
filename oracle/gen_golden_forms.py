"""Golden vectors at the form boundaries of ksw_exts2_sse, ksw_extf2_sse and the SSE-compatible mode (tests/form_edge_util.py): a
fixed subset of those grids -- at least one case per kernel form and per side of each admission limit, for exts every mode at
min(qlen, tlen) = 448 / 449 and 960 / 961 -- with every ksw_extz_t field and the CIGAR of the UNMODIFIED reference, the switches
each case runs under and the form it expects.

Run in the build container only (needs oracle/_ref):   python oracle/gen_golden_forms.py   ->   tests/golden/form_edge_cases.npz
The file is data only and reproducible: a second run writes the same bytes.
"""
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import form_edge_util as fe                  # noqa: E402

FIELDS = ["score", "max", "max_t", "max_q", "mqe", "mqe_t", "mte", "mte_q", "zdropped", "reach_end", "n_cigar"]   # = tests/golden_util.FIELDS
MAX_BYTES = 437684                                      # the largest fixture committed before this one (random_cases.npz)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member times, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(zi, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def main():
    cases = fe.golden_subset()
    seqs, seq_off, params, expect, cigs, cig_off, grp_id = [], [0], [], [], [], [0], {}
    none = np.zeros(0, dtype=np.uint8)
    for c in cases:
        res = fe.reference(c, "ref")
        j = none if c["junc"] is None else c["junc"]
        for s in (c["q"], c["t"], j):
            seqs.append(s)
            seq_off.append(seq_off[-1] + len(s))
        g = grp_id.setdefault((c["fam"], c["grp"]), len(grp_id))
        params.append([fe.FAMS.index(c["fam"]), c["dual"], c["m"], *c["sc"], c["w"], c["zdrop"], c["flag"], c["jb"], c["env"], fe.WANTS.index(c["want"]), g])
        expect.append([res[f] for f in FIELDS])
        cigs += res["cigar"]
        cig_off.append(len(cigs))
    out = os.path.join(ROOT, "tests", "golden", "form_edge_cases.npz")
    write_npz(out, dict(seq=np.concatenate(seqs).astype(np.uint8), seq_off=np.array(seq_off, dtype=np.int64), params=np.array(params, dtype=np.int32),
                        expect=np.array(expect, dtype=np.int64), cigar=np.array(cigs, dtype=np.uint32), cigar_off=np.array(cig_off, dtype=np.int64)))
    size = os.path.getsize(out)
    assert size <= MAX_BYTES, size
    ex = np.array(expect)
    print("wrote", len(cases), "cases,", size, "bytes; by family", {f: sum(1 for c in cases if c["fam"] == f) for f in fe.FAMS},
          "zdropped", int(ex[:, 8].sum()), "with CIGAR", int((ex[:, 10] > 0).sum()))


if __name__ == "__main__":
    main()
