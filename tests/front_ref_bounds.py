"""Measured differences between the restatements of the EKF fusion and the reference's own build
(tests/golden/front_ref_golden.npz), and the bounds the tests derive from them.  DESIGN.md section 2, table
"front-end pins", summarises these numbers; `python tests/test_front_ref_pins.py` prints them as measured now.

Scaling as tests/test_gpu_fuse.py:72-74: `fused` per entry by max(1, |reference|) (m, m, degrees), `cov` by the largest
|entry| of the reference's covariance.  A bound is 4 x the measured value -- room for another compiler version's choice
of evaluation order on a handful of multiply-adds, not for a wrong term -- and 0 where every vector was bit-equal.  For
the C oracle it is never looser than what tests/test_gpu_fuse.py allows between oracle and device (fused 1e-10,
cov 1e-12 x scale).  The mirror (replay.PoseFuser) and the numpy twin invert with np.linalg.inv (LU with pivoting)
where Eigen and the oracle use cofactors: their difference grows with the condition number of the Hessian.
"""
import math

FACTOR = 4.0
ORACLE_CAP = (1e-10, 1e-12)          # tests/test_gpu_fuse.py:73-74, oracle against device
DEVICE_FUSED_TOL, DEVICE_COV_REL, DEVICE_COV_ABS = 1e-10, 1e-9, 1e-12     # the same lines, as the GPU pins add them

# The twin and the mirror multiply and invert through numpy, whose BLAS / LAPACK picks its kernels (and with them the
# order of a 3-term sum and the use of fused multiply-adds) by the CPU it runs on: where they happened to be bit-equal
# here, 4 x 0 would assert an evaluation order nobody chose.  Their bounds are therefore never below 16 ulp of the
# scaled quantity -- a 3x3 product chain of five factors rounds about that often; a wrong term is 1e10 times larger.
# The C oracle is compiled without contraction and gets no such floor.
NUMPY_FLOOR = 16 * 2.220446049250313e-16

# {restatement: {floor(log10(cond(H))): (fused, cov)}} over the finite fusion vectors
FUSION = {
    'oracle': {0: (0, 5.23e-14), 1: (1.82e-16, 2.14e-14), 2: (0, 1.07e-15), 3: (0, 1.43e-16), 4: (0, 8.06e-15), 5: (0,
        3.52e-16), 6: (0, 1.55e-16), 7: (0, 1.11e-15), 8: (0, 9.64e-15), 9: (0, 2.35e-16), 10: (0, 3.99e-16)},
    'twin': {0: (5.77e-15, 1.49e-12), 1: (1.88e-15, 4.36e-12), 2: (2.2e-15, 8.9e-15), 3: (2.24e-16, 3.19e-15), 4:
        (3.21e-15, 3.19e-13), 5: (7.39e-13, 7.83e-12), 6: (1.09e-13, 7.34e-11), 7: (1.12e-09, 2.57e-08), 8: (3.09e-09,
        4.31e-07), 9: (2.36e-09, 2.29e-07), 10: (1.31e-07, 3.53e-05)},
    'replay': {0: (2.38e-16, 2.05e-12), 1: (2.78e-16, 1.48e-11), 2: (3.14e-16, 8.03e-15), 3: (2.22e-16, 2.95e-15), 4:
        (3.36e-15, 3.19e-13), 5: (7.37e-13, 7.83e-12), 6: (1.1e-13, 7.34e-11), 7: (1.12e-09, 2.57e-08), 8: (3.09e-09,
        4.31e-07), 9: (2.36e-09, 2.29e-07), 10: (1.31e-07, 3.53e-05)},
}
# {restatement: [(fused, cov) per step of the chained run, own outputs fed back]}
CHAIN = {
    'oracle': [(0, 0), (0, 9.61e-17), (0, 9.64e-16), (0, 5.89e-17), (0, 5.6e-15), (1.11e-16, 2.09e-14), (0, 5.15e-15),
        (0, 1.83e-15), (0, 3.83e-16), (0, 4.41e-15), (0, 1.16e-15), (0, 5.22e-16), (0, 3.14e-16), (0, 2.15e-16), (0,
        2.41e-13), (0, 4.37e-15), (1.56e-16, 5.9e-14), (2.12e-16, 2.02e-15), (1.94e-16, 2.82e-16), (2.12e-16,
        5.52e-14), (0, 3.24e-13), (1.49e-16, 1.52e-13), (0, 9.81e-15), (0, 1.96e-16), (0, 2.84e-14), (1.24e-16,
        1.31e-13), (1.28e-16, 2.36e-13), (1.84e-16, 1.8e-15), (1.8e-16, 6.72e-16), (2.75e-16, 2.83e-13), (0,
        2.32e-15), (0, 1.72e-15), (0, 8.48e-15), (0, 6.11e-17), (0, 1.94e-15), (0, 2.44e-13), (0, 8.52e-16), (0,
        4.47e-13), (0, 4.42e-16), (0, 2.42e-14), (0, 5.52e-14), (0, 1.97e-14), (0, 4.16e-15), (0, 4.26e-16), (0,
        1.38e-15), (0, 1.26e-14), (0, 1.89e-14), (1.75e-16, 4.52e-15), (1.72e-16, 4.6e-16), (0, 3.17e-15), (0,
        7.27e-14), (0, 1.21e-15), (0, 4.13e-13), (0, 5.23e-15), (3.65e-16, 6.56e-13), (1.37e-16, 9.74e-15), (1.2e-16,
        2.13e-13), (1.44e-16, 7.13e-13), (3.61e-16, 3.72e-15), (3.73e-16, 2.52e-15)],
    'twin': [(0, 3.89e-16), (1.63e-16, 9.61e-17), (3.2e-16, 4.93e-15), (3.33e-16, 1.3e-15), (3.21e-16, 1.33e-14),
        (3.24e-16, 1.08e-14), (3.33e-16, 3.37e-15), (3.33e-16, 2.2e-15), (4.4e-16, 5.1e-16), (4.14e-16, 2.27e-15),
        (3.89e-16, 6.45e-16), (3.6e-16, 2.61e-16), (3.28e-16, 1.57e-16), (2.95e-16, 2.15e-16), (0, 4.87e-14),
        (1.95e-16, 2.59e-15), (1.56e-16, 3.71e-14), (2.12e-16, 8.97e-16), (1.94e-16, 1.46e-16), (1.24e-16, 1.16e-14),
        (0, 2.29e-13), (2.22e-16, 1.36e-13), (3.41e-16, 6.13e-15), (3.5e-16, 1.37e-15), (0, 2.64e-14), (2.48e-16,
        8.62e-14), (2.56e-16, 4.14e-13), (1.31e-16, 4.33e-15), (1.35e-16, 8.96e-16), (4.13e-16, 2.4e-13), (1.42e-16,
        2.32e-15), (0, 3.29e-15), (0, 3.64e-14), (0, 3.26e-16), (1.58e-16, 1.94e-15), (3.29e-16, 7.58e-14), (0,
        1.56e-15), (0, 8.15e-14), (0, 1.11e-16), (0, 2.42e-14), (1.99e-16, 6.98e-14), (4.17e-16, 1.43e-14), (4.4e-16,
        1.64e-15), (4.63e-16, 6.39e-16), (0, 5.52e-15), (2.6e-16, 1.1e-14), (2.73e-16, 9.46e-15), (2.83e-16,
        2.74e-14), (3.02e-16, 2.66e-15), (1.69e-16, 6.34e-15), (3.52e-16, 2.16e-13), (1.88e-16, 2.55e-15), (0,
        2.16e-13), (0, 2.74e-15), (0, 3.42e-13), (0, 7.77e-15), (1.59e-16, 1.63e-13), (1.79e-16, 1.01e-12), (3.61e-16,
        5.14e-15), (2.49e-16, 4.83e-15)],
    'replay': [(0, 3.89e-16), (0, 1.92e-16), (0, 4.07e-15), (0, 2.36e-16), (0, 2.39e-14), (1.11e-16, 2.2e-14), (0,
        4.36e-15), (0, 2.08e-15), (0, 5.1e-16), (0, 2.54e-15), (0, 6.45e-16), (0, 2.61e-16), (0, 1.57e-16), (0,
        2.15e-16), (0, 4.87e-14), (0, 2.59e-15), (1.56e-16, 4.24e-14), (2.12e-16, 3.14e-15), (1.94e-16, 5.64e-16),
        (2.12e-16, 3.89e-14), (0, 2.17e-13), (0, 2.81e-13), (0, 7.34e-15), (0, 1.96e-16), (0, 9.32e-14), (0,
        7.59e-14), (0, 4.02e-13), (0, 4.33e-15), (0, 6.72e-16), (2.75e-16, 1.17e-13), (0, 2.61e-15), (0, 5.17e-15),
        (1.49e-16, 6.31e-14), (1.54e-16, 4.89e-16), (0, 1.02e-15), (0, 4.21e-14), (0, 1.28e-15), (0, 7.75e-14), (0,
        1.47e-16), (0, 1.73e-14), (0, 7.31e-14), (0, 8.77e-15), (0, 1.64e-15), (0, 2.13e-16), (0, 3.05e-15),
        (1.85e-16, 4.76e-15), (2.16e-16, 1.5e-14), (1.75e-16, 2.98e-14), (1.72e-16, 3.48e-15), (0, 5.4e-15), (0,
        4.22e-13), (0, 1.34e-15), (0, 4.73e-13), (0, 5.66e-15), (3.65e-16, 1.65e-13), (1.37e-16, 3.42e-15), (0,
        9.26e-14), (1.44e-16, 5.6e-13), (3.61e-16, 2.84e-15), (3.73e-16, 5.25e-15)],
}


def decade(cond):
    """Condition-number decade of a Hessian: floor(log10(cond)), with 10^d itself (computed to ~1e-6) counted to d."""
    return int(math.floor(math.log10(cond) + 0.005))


def _bound(name, measured):
    bf, bc = FACTOR * measured[0], FACTOR * measured[1]
    if name == "oracle":
        bf, bc = min(bf, ORACLE_CAP[0]), min(bc, ORACLE_CAP[1])
    else:
        bf, bc = max(bf, NUMPY_FLOOR), max(bc, NUMPY_FLOOR)
    return bf, bc


def fusion_bound(name, dec):
    return _bound(name, FUSION[name][dec])


def chain_bound(name, k):
    return _bound(name, CHAIN[name][k])
