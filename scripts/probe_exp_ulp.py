#!/usr/bin/env python3
"""Measure the error of the exponential that csr5hip_row_softmax uses, through the entry point itself.

    python scripts/probe_exp_ulp.py [--rows 1048576] [--seed 1]

Runs the softmax on 2**20 rows of two entries (d, 0), d seeded over (-745, 0] for fp64 and (-103, 0] for fp32.  For such a row
d - M = d is exact; besides the exponential the first output holds one rounded addition (1 + exp(d)) and the two roundings of
the quotient (one reciprocal, one multiplication).  E = max |out_0 - ref| / (u ref) against the long double reference
therefore bounds the exponential's error in units of u from above; tests/softmax_reference.py takes C_EXP = ceil(E).
References below the smallest normal number are left out (the bound of the tests does not judge them either).
Prints one JSON line per value type.  Needs a GPU."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    from benchmark_spmv_using_csr5_amd import handle as H
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63
    dev = "cuda:0"
    m = args.rows
    row_ptr = torch.arange(0, 2 * m + 1, 2, dtype=torch.int32, device=dev)
    col = torch.zeros(2 * m, dtype=torch.int32, device=dev)
    for dtype, lo in ((np.float64, -745.0), (np.float32, -103.0)):
        rng = np.random.default_rng([args.seed, np.dtype(dtype).itemsize])
        # half of the draws uniform over the whole span, half over (-1, 0] where exp(d) weighs most in the quotient
        d = np.where(rng.random(m) < 0.5, rng.uniform(lo, 0.0, size=m), -rng.random(m)).astype(dtype)
        s = np.zeros(2 * m, dtype=dtype)
        s[0::2] = d
        sd = torch.from_numpy(s).to(dev)
        out = torch.empty_like(sd)
        A = H.anonymouslibHandle(m, 1, dtype=np.dtype(dtype).name)
        assert A.inputCSR(2 * m, row_ptr, col, torch.zeros_like(sd)) == 0
        assert A.rowSoftmax(sd, out) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(LD)
        A.close()
        ex = np.exp(d.astype(LD))
        Z = ex + 1
        u = LD(np.finfo(dtype).eps) / 2
        tiny = LD(np.finfo(dtype).tiny)
        res = {"dtype": np.dtype(dtype).name, "rows": m}
        for name, o, ref in (("E", got[0::2], ex / Z), ("E_other_entry", got[1::2], 1 / Z)):
            keep = ref >= tiny
            err = np.abs(o[keep] - ref[keep]) / (u * ref[keep])
            i = int(np.argmax(err))
            res[name] = float(err.max())
            res[name + "_at_d"] = float(d[keep][i])
        res["C_EXP"] = int(math.ceil(res["E"]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
