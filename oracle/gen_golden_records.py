#!/usr/bin/env python3
"""Record what the REFERENCE's own code outputs for the tests that compare against it live (TEST INFRASTRUCTURE ONLY).

Those tests run the live reference (oracle/_ref) where it is built and this record everywhere else, so that they stand
without the reference's sources.  Written to tests/golden/reference_records.json:

  * cli.<fixture>   -- exit code of the reference CLI (CSR5_avx2/main.cpp through oracle/_ref/libref_ingest.so) on
                       each readable, non-empty tests/golden/mtx/<fixture>.mtx, and the lines of its stdout that carry no time or path
                       (precision, dimensions, omega / sigma / #partition, its own self-check);
  * zoo.<matrix>|w<omega>|s<sigma> -- sha256 of each CSR5 array the reference's format code builds for the test zoo
                       (masked as tests/test_oracle_golden.py::assert_format_equal compares them) and of the rows of
                       CSR5_avx2's y that have non-zeros, on the reference CLI's integer data.

Runs only where oracle/_ref/*.so exist (`make -C oracle ref`).  Re-run:  python oracle/gen_golden_records.py
"""
import glob
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from oracle.csr5_oracle import Reference  # noqa: E402
from tests import zoo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_records.json")
MTX_DIR = os.path.join(ROOT, "tests", "golden", "mtx")
ZOO_OMEGAS = (4, 32, 64)
ZOO_SIGMAS = (4, 5, 12, 16, 17, 32)
ZOO_VALUE_SEED = 21


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cli_facts(text: str) -> list:
    """The stdout lines of the reference CLI that are the same on every run and every machine."""
    return [l for l in text.splitlines() if l.strip() and "time" not in l and not l.startswith("-")]


def format_digest(f, written=None) -> dict:
    """Digests of a Csr5Format as assert_format_equal compares it; `written`: the offset slots the reference wrote."""
    p = f.p
    tp = f.tile_ptr.copy()
    tp[p - 1] &= 0x7FFFFFFF
    n = (p - 1) * f.omega * f.num_packet
    written = f.offset != -1 if written is None else written
    return {"params": [int(f.bit_y), int(f.bit_ss), int(f.num_packet), int(p), int(f.num_offsets), int(f.tail_start)],
            "tile_ptr": sha(tp), "tile_desc": sha(f.tile_desc[:n]), "offset_ptr": sha(f.offset_ptr),
            "offset_written": sha(np.flatnonzero(written)), "offset": sha(f.offset[written]),
            "col": sha(f.col), "val": sha(f.val)}


def y_digest(mat, y) -> str:
    return sha(np.asarray(y, dtype=np.float64)[np.diff(mat.row_ptr) > 0])


def main():
    assert Reference.ingest_available() and Reference.available() and all(Reference.available(w) for w in ZOO_OMEGAS), \
        "oracle/_ref is missing: run `make -C oracle ref` where the reference's sources are"
    ref = Reference()
    rec = {"cli": {}, "zoo": {}}
    expected = np.load(os.path.join(MTX_DIR, "expected.npz"))
    for path in sorted(glob.glob(os.path.join(MTX_DIR, "*.mtx"))):
        name = os.path.basename(path)[:-4]
        if int(expected[name + ".code"]) != 0 or name == "empty_matrix":  # (the CLI is run on readable, non-empty files only)
            continue
        rc, text = ref.cli(path)
        rec["cli"][name] = {"rc": rc, "lines": cli_facts(text)}
    for mat in zoo.small_zoo():
        val, x = M.fill_values(mat.nnz, mat.n, np.float64, seed=ZOO_VALUE_SEED, mode="int")
        for omega in ZOO_OMEGAS:
            for sigma in ZOO_SIGMAS:
                rec["zoo"][f"{mat.name}|w{omega}|s{sigma}"] = format_digest(
                    ref.convert(omega, sigma, mat.m, mat.row_ptr, mat.col, val))
        y, _, _ = ref.avx2_spmv(mat.m, mat.n, mat.row_ptr, mat.col, val, x, y0=np.full(mat.m, 777.0))
        rec["zoo"][f"{mat.name}|y_avx2"] = y_digest(mat, y)
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"wrote {OUT}: {len(rec['cli'])} CLI runs, {len(rec['zoo'])} zoo records")


if __name__ == "__main__":
    main()
