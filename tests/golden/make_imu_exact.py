#!/usr/bin/env python3
"""Generate tests/golden/imu_exact.npz: the exact pre-integration row (tests/imu_exact.py, mpmath at 50 digits) of every interval in
tests/imu_cases.py, as double-double pairs (hi = float(x), lo = float(x - hi)), with a digest of each interval's inputs and the inputs
themselves for the intervals small enough to carry (the large ones are regenerated from imu_cases.py and checked by digest).

    python tests/golden/make_imu_exact.py          # rewrites tests/golden/imu_exact.npz; about a minute (20 ms per IMU sample)

tests/test_imu_exact.py recomputes every interval of at most imu_cases.REGEN_MAX_SAMPLES samples and requires equality with the file."""
import os
import sys
import time
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import imu_cases
import imu_exact

INPUT_KEYS = ("noise", "acc_0", "gyr_0", "ba", "bg", "dt", "acc", "gyr")


def exact_row(case):
    """(hi[467], lo[467]) of one interval"""
    return imu_exact.to_dd(imu_exact.preintegrate_exact(*[case[k] for k in INPUT_KEYS]))


def main():
    out = {}
    names = []
    for name, case in imu_cases.intervals().items():
        t0 = time.time()
        hi, lo = exact_row(case)
        names.append(name)
        out["hi/" + name], out["lo/" + name] = hi, lo
        out["digest/" + name] = np.array(imu_cases.digest(case))
        if len(case["dt"]) <= imu_cases.REGEN_MAX_SAMPLES:
            for k in INPUT_KEYS:
                out["in/%s/%s" % (name, k)] = np.asarray(case[k], dtype=np.float64)
        print("%-20s %5d samples  %6.1f s  sum_dt = %r" % (name, len(case["dt"]), time.time() - t0, hi[0]))
    out["names"] = np.array(names)
    path = os.path.join(HERE, "imu_exact.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
