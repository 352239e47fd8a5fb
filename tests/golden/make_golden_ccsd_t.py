"""Stored references of the (T) cases that run at the production tile, wave counts and buffer caps (tests/ccsd_t_cases.py: PIN_CASES and PRODUCTION_PIN;
tests/test_gpu_ccsd_t.py and tests/test_ccsd_t_hostlogic.py compare the device and the scalar mock against them).

For every pinned (o, v): the slab-wise twin tests/ccsd_t_numpy.py::slabbed on tn.random_system(o + v, o, 1000 o + v, scale=0.1), the family of
ccsd_t_cases.system.  Stored: o, v, e_t, abs_sum, one entry per shape -- a few hundred bytes.  The twin needs seconds per shape up to (21, 19) and about
four minutes at (20, 64) on a handful of cores (five minutes in all), too long for a GPU test, hence stored; the CPU file recomputes every shape but (20, 64)
and holds the file to the twin (test_stored_pins_are_the_twin).

    python tests/golden/make_golden_ccsd_t.py        (writes tests/golden/ccsd_t_pins.npz)
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "oracle"))
import ccsd_t_cases as tc  # noqa: E402
import ccsd_t_numpy as tn  # noqa: E402


def main():
    rows = []
    for o, v in tc.pinned_shapes():
        t0 = time.time()
        ref = tn.slabbed(*tc.pin_inputs(o, v))
        rows.append((o, v, ref["e_t"], ref["abs_sum"]))
        print(f"({o}, {v}): e_t = {ref['e_t']!r} abs_sum = {ref['abs_sum']!r} ({time.time() - t0:.1f} s)", flush=True)
    o, v, e_t, abs_sum = zip(*rows)
    np.savez(ROOT / "tests" / "golden" / "ccsd_t_pins.npz", o=np.array(o, dtype=np.int64), v=np.array(v, dtype=np.int64), e_t=np.array(e_t), abs_sum=np.array(abs_sum))


if __name__ == "__main__":
    main()
