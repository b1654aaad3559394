"""What tests/test_subspace_host.py and tests/test_gpu_subspace.py share: the dense model's matrix, and the iteration count the host test
finds for it and the device tests run for."""
import numpy as np

# The dense model on model_h() with random trial vectors reaches the three lowest eigenvalues to 1e-9 after 240 iterations (6.1e-10, the
# matrices of the last 5 iterations averaged) and to 8.3e-11 after 260; 220 leave 4.5e-9.  260 it is: tests/test_gpu_subspace.py runs
# the device loop for the same count.
N_ITER, BURN_IN = 260, 255
MODEL_EPS, MODEL_RESTART = 0.1, 5


def model_h():
    """A random symmetric 40 x 40 matrix (GOE, seed 68: of seeds 0 .. 399 the one whose third and fourth eigenvalues lie furthest
    apart, which is what the iteration count depends on) and three random trial vectors"""
    rng = np.random.RandomState(68)
    a = rng.standard_normal((40, 40))
    return (a + a.T) / 2, rng.standard_normal((3, 40))
