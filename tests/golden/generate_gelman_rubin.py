#!/usr/bin/env python3
"""
Generate tests/golden/gelman_rubin.npz by running the reference's own ``gelman_rubin`` function.

    python tests/golden/generate_gelman_rubin.py REFERENCE_DIR

REFERENCE_DIR is a checkout of the reference project (it holds ``gelman_rubin.py``).  The fixture stores the seed, the
shape and the reference's R-hat only; tests/chain_reference.py:gelman_rubin_input regenerates the input from the seed.
The shape is the one the reference's scripts pass: ``sampler.get_chain(discard=..., flat=False)``, (steps, walkers, ndim).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, SHAPE = 20240607, (300, 48, 4)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path[:0] = [os.path.abspath(sys.argv[1]), os.path.dirname(HERE)]
    from gelman_rubin import gelman_rubin  # the reference's function
    from chain_reference import gelman_rubin_input

    rhat = gelman_rubin(gelman_rubin_input(SEED, SHAPE))
    np.savez(os.path.join(HERE, "gelman_rubin.npz"), seed=np.int64(SEED), shape=np.array(SHAPE, dtype=np.int64), rhat=rhat)
    print("gelman_rubin.npz:", rhat)


if __name__ == "__main__":
    main()
