#!/usr/bin/env python3
"""The bf16x6 kernels (fp32 operands as three bf16 pieces, six piece products) against fp64, from the case modules the tests use
(tests/bf16x6_cases.py, tests/bf16x6_only_cases.py: no second copy of the cases here).

* The kernels that have an exact-fp32 twin (dmp_dev_set_exact_fp32(1): v_mfma_f32_32x32x2_f32), at H = 128 and H = 64: per scenario and
  kernel ``[bf16x6 error, exact-fp32 error, finite]`` -- of the element's natural scale, sum_k |a_k| |b_k|, on the adversarial operands;
  of the element itself on the sparse ladder.
* The kernels that have none: per kernel, scenario and output the error, the derived fp32 bound and, where the kernel replaces launches
  that have an exact form, those launches' error under the switch.

Prints one JSON document; ``--out FILE`` writes it there as well (profiles/bf16x6_envelope.json is such a run on an MI355X)."""
import argparse
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON document to this file")
    args = ap.parse_args()
    from bf16x6_cases import ROWS, run_all
    from bf16x6_only_cases import run_only
    gpu = th.device("cuda:0")
    doc = {"device": th.cuda.get_device_name(0), "with_an_exact_form": {}, "bf16x6_only": run_only(gpu)}
    for h in sorted(ROWS, reverse=True):
        doc["with_an_exact_form"]["H=%d rows=%d" % (h, ROWS[h])] = run_all(gpu, h=h)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
