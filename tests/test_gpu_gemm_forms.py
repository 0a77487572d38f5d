"""GPU: the generic GEMM (csrc/gemm.hip launch_gemm) on each of its ten kernel instantiations — gemm_split/64, gemm_split/128,
gemm_fast/64, gemm_fast/128 and gemm_f32, each with trans_b 0 and 1 — against the float64 evaluation of tests/gemm_cases.py, through
bsg_gemm_ex (force_form picks the kernel where the dispatch would pick by workgroup count; no model of the suite is large enough to
reach the 128-row tiles otherwise).

Sentinels.  Every operand is a window inside a larger buffer whose surroundings are NaN: the lda - K / ldb - K padding columns, the
gaps between batch items and between taps, taps / 2 + 1 rows before A's first and after its last item (so a tap that leaves its item
reads NaN in the windowed layouts and the neighbour's rows in the dense ones), and the same around bias_m, bias_n, post_scale_n /
post_shift_n, R and rowscale.  A load that is masked only after the multiply turns the result NaN; a NaN that a split form stages
also counts as a range event.  C is a window (ldc > N, sC > M * ldc) in a buffer filled with one bit pattern: after the call every
element outside the M x N windows still holds it, bit for bit.  The `tight` cases are the consumers' dense layouts.

Bars, for every case: the suite's ceiling for unit-normal operands, 2e-6 * 4 * sqrt(K * taps) + 1e-5, and 2 x the deviation of
gemm_ref(float32) from gemm_ref(float64) + 2e-5 x the result's scale (the floor of tests/test_gpu_f2_fullsize.py).

Every test prints, per instantiation, the largest hip deviation, the largest deviation of the float32 reference and the largest
deviation / bar of a single case.  The measured table is not recorded here yet: no MI355X run of this file was available when it was
written (the layouts, the descriptor and the reference were checked against each other on the CPU, tests/test_gemm_cases_cpu.py).
"""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = 0x7fc5a5a5            # C's fill: a NaN with a payload no arithmetic produces
ALIGNED_FORMS = ('gemm_split/64', 'gemm_split/128', 'gemm_fast/64', 'gemm_fast/128')
INSTANCES = [(f, tb) for f in gc.FORMS for tb in (1, 0)]
_inst_id = lambda v: f'{gc.FORMS[v[0]]}/trans_b{v[1]}'


def run(c, ops, force, **over):
    """Lay the operands out, call bsg_gemm_ex, check C's surroundings -> (C windows [nz, M, N] float64 numpy, name of the form)."""
    L, host, offs, n_c, c_pre, inside, idx = gc.pack(c, ops, **over)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    cbuf = torch.full((n_c,), SENTINEL, dtype=torch.int32, device='cuda')
    p = lambda k: (dev[k].data_ptr() + 4 * offs[k]) if k in dev else None
    d = _lib.GemmDesc(A=p('A'), B=p('B'), C=cbuf.data_ptr() + 4 * c_pre, bias_m=p('bias_m'), bias_n=p('bias_n'), post_scale_n=p('post_scale_n'),
                      post_shift_n=p('post_shift_n'), R=p('R'), rowscale=p('rowscale'), **gc.desc_scalars(c, L))
    form = ctypes.c_char_p()
    _lib.check(_lib.load().bsg_gemm_ex(ctypes.byref(d), force, ctypes.byref(form), _lib.stream_ptr()), f'bsg_gemm_ex {c.name}')
    torch.cuda.synchronize()
    bits = cbuf.cpu().numpy()
    assert (bits[~inside] == SENTINEL).all(), f'{c.name}: {int((bits[~inside] != SENTINEL).sum())} elements outside the C windows were written'
    return bits.view(np.float32)[idx].astype(np.float64), form.value.decode()


_REFS = {}


def reference(c):
    """(operands, float64 reference, deviation of the float32 reference from it, scale): computed once per case, shared by the forms."""
    if c not in _REFS:
        ops = gc.operands(c)
        r64 = gc.gemm_ref(c, ops, torch.float64)
        r32 = gc.gemm_ref(c, ops, torch.float32)
        r64.setflags(write=False)
        _REFS[c] = (ops, r64, float(np.abs(r32 - r64).max()), max(1.0, float(np.abs(r64).max())))
    return _REFS[c]


@pytest.fixture(autouse=True)
def _clean_range_word():
    _lib.gemm_range_take()
    yield


def check(c, force, stats=None, **over):
    ops, r64, dev32, scale = reference(c)
    got, form = run(c, ops, force, **over)
    if force:
        assert form == gc.FORMS[force], (c.name, form)
    assert np.isfinite(got).all(), f'{c.name} on {form}: {int((~np.isfinite(got)).sum())} non-finite results'
    dev = float(np.abs(got - r64).max())
    bar = min(gc.ceiling(c), 2 * dev32 + 2e-5 * scale)
    if stats is not None:
        stats.append((dev, dev32, dev / bar, c.name))
    assert dev <= gc.ceiling(c), (c.name, form, dev, gc.ceiling(c))
    assert dev <= 2 * dev32 + 2e-5 * scale, (c.name, form, dev, dev32, scale)
    if form.startswith('gemm_split'):
        assert _lib.gemm_range_take() == 0, f'{c.name} on {form}: in-range operands raised a range event'
    return form


def _report(what, inst, stats):
    dev, dev32, ratio = (max(s[i] for s in stats) for i in range(3))
    worst = max(stats, key=lambda s: s[2])[3]
    print(f'gemm forms, {what}, {_inst_id(inst)}: {len(stats)} cases, hip {dev:.2e}, fp32 yardstick {dev32:.2e}, ratio {ratio:.3f} ({worst})')


@pytest.mark.parametrize('inst', INSTANCES, ids=_inst_id)
def test_shape_sweep(inst):
    """Tile edges in M, N and K, taps wider than the item, batch and the two-level batch, with every epilogue option on."""
    stats = []
    for c in gc.sweep_cases(*inst):
        check(c, inst[0], stats)
    _report('shape sweep', inst, stats)


@pytest.mark.parametrize('force', list(gc.FORMS), ids=lambda f: gc.FORMS[f])
def test_consumer_patterns(force):
    """The pitch extractor's k = 5 convolution (T = 5 and 129, K = 80 and 256, batch 3, ReLU, post-affine, row mask with sRS = T), its N = 2
    Linear with ldc = 2 and the batched bias_n, in the dense layouts the consumers pass: a tap that leaves its batch item reads the
    neighbour's rows here, a row mask with the wrong batch stride the neighbour's mask."""
    stats = []
    for c in gc.consumer_cases():
        check(c, force, stats)
    _report('consumer patterns', (force, 1), stats)


@pytest.mark.parametrize('inst', INSTANCES, ids=_inst_id)
def test_epilogue_sweep(inst):
    """Each epilogue option alone, then all together, on a whole-tile shape and on one with partial tiles in M, N and K."""
    stats = []
    for c in gc.epilogue_cases(inst[1]):
        check(c, inst[0], stats)
    _report('epilogue sweep', inst, stats)


@pytest.mark.parametrize('kind', list(gc.UNALIGNED))
def test_auto_dispatch_takes_gemm_f32_when_unaligned(kind):
    c, over = gc.UNALIGNED[kind]
    assert check(c, 0, **over) == 'gemm_f32'


@pytest.mark.parametrize('trans_b', [1, 0])
def test_auto_dispatch_takes_an_aligned_form_when_aligned(trans_b):
    c = replace(gc.AUTO, trans_b=trans_b)
    assert check(c, 0) in ALIGNED_FORMS
    # N % 4 != 0 breaks the rule only for trans_b = 0
    if trans_b:
        assert check(replace(gc.AUTO, N=38), 0) in ALIGNED_FORMS


def test_forced_aligned_form_on_unaligned_problem_is_refused():
    c, over = gc.UNALIGNED['lda%4']
    ops = reference(c)[0]
    for force in (1, 2, 3, 4):
        with pytest.raises(_lib.BsgError, match='aligned'):
            run(c, ops, force, **over)
