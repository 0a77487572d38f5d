"""The ragged pitch-extractor cases shared by tests/test_pe_ragged_cpu.py (the float64 oracle alone decides every row) and
tests/test_gpu_pe_ragged.py.  B = 4 rows, seed 1900 + T; the lengths put a row's end on, before and after the 64-frame seams of
positions_kernel and the GEMM tiles (65 / 64 / 63, 129 / 128 / 127), below the 64 frames at which groupnorm_res_kernel has a float4 per
thread, and below the five taps (5, 3, 2, 1).  No GPU is needed to import this module."""
import numpy as np

from tests import pe_cases

CASES = [(129, [129, 65, 64, 5]), (70, [70, 63, 2, 1]), (257, [257, 128, 127, 3])]
IDS = [f'T{T}' for T, _ in CASES]
B = 4


def mel(T, lens):
    """[4, T, 80] float32, exactly 0 from frame lens[b] on: the padded batch as forward_batch hands it over."""
    return pe_cases.mel(np.random.RandomState(1900 + T), B, T, lens)


def nan_tail(m, lens):
    """The same batch with NaN at and beyond each row's end: what a ragged call must never read."""
    m = m.copy()
    for b, n in enumerate(lens):
        m[b, n:] = np.nan
    return m
