"""Generic inputs of the correctly rounded exp (csrc/nk_exp.h) that its fast phase does not settle
-> tests/golden/exp_ziv.npz.

The fast phase's rounding test hands about 2^-18 of the inputs of the Bratu range to the exact
fixed-point phase.  This scans uniform [-1, 3] in blocks until at least 48 of them are found
(oracle.exp_rare: where nkx_exp_fast returns 0 -- the source the device compiles, so the decision the
device makes) and stores them with exp(x) from mpmath at 250 bits rounded once to binary64
(make_exp_golden.cr_exp).  Unlike the family x = a 2^-52 + 2^-53 these are ordinary field values:
tests/test_hip_exp_rare.py plants them in the Bratu grids, and tests/test_exp.py holds that they still
take the exact phase (so those tests do not lose their coverage to a later change of nk_exp.h).

    python tests/golden/make_exp_ziv.py        (deterministic: numpy default_rng(2027))
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_exp_golden import cr_exp  # noqa: E402
from oracle import oracle as oc  # noqa: E402

WANT, BLOCK = 48, 2_000_000


def inputs(seed=2027):
    rng = np.random.default_rng(seed)
    found = []
    while sum(len(f) for f in found) < WANT:
        x = rng.uniform(-1.0, 3.0, BLOCK)
        found.append(x[oc.exp_rare(x)])
    return np.concatenate(found)


def main():
    x = inputs()
    y = np.array([cr_exp(v) for v in x])
    np.savez_compressed(os.path.join(HERE, "exp_ziv.npz"), x=x, y=y)
    print(f"{len(x)} vectors -> exp_ziv.npz")


if __name__ == "__main__":
    main()
