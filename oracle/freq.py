"""Inverse frequencies of the sinusoidal tables: fs2.sinusoidal_table, fs2.rel_pos_table and diffnet.sinusoidal_pos_emb."""
import torch


def inv_freq(exponent):
    """exp() of a float32 exponent vector, in float32 as the reference evaluates it.  The last bit of a float32 exp follows the host's
    math library (MKL takes other code paths on other CPUs), and row p of a table multiplies that bit by p: one ulp moves row 64 of the
    decoder's position table by ~4e-6.  tests/test_oracle_golden.py therefore evaluates the oracle with the vectors of the host that made
    the goldens (tests/golden/inv_freq.npz) and holds this function to one ulp of them."""
    return torch.exp(exponent)
