"""CPU: what the ragged FastSpeech2 front (ABI v20) rests on, without a GPU — the "alone" oracle of tests/fs2_ragged_cases.py, the two-row
table form of the ESM, the cases' power to tell the padded front from the utterance alone, the bounds, the refusals that need no device
and the ABI entries.  The GPU side is tests/test_gpu_fs2_ragged.py."""
import os
import re

import pytest
import torch

from bisinger_amd import _lib
from oracle import fs2 as ofs2
from tests import fs2_ragged_cases as RC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def ref(c):
    """One evaluation per case, shared and left unchanged: (tensors, alone float64, alone float32)."""
    if c.name not in _REF:
        _, hp, sd = RC.model(c.front, c.depth)
        t = RC.tensors(RC.inputs(c))
        _REF[c.name] = (t, RC.alone(sd, hp, c, t, RC.F64), RC.alone(sd, hp, c, t, RC.F32))
    return _REF[c.name]


def test_esm_alone_is_the_two_row_table():
    """At B = 1 the ESM's attention over the batch axis has one key: the whole module is a function of the token's lang id."""
    _, hp, sd = RC.model('midi', 2)
    table = RC.esm_table(sd, 'fs2.esm.', RC.F64)
    assert table.shape == (2, 256)
    g = torch.Generator().manual_seed(3)
    lang = torch.randint(0, 2, (1, 37), generator=g)
    Eo = torch.randn(1, 37, 256, generator=g, dtype=RC.F64) * 3      # the token embedding: Q only, which drops out
    LP = torch.nn.functional.embedding(lang, sd['fs2.lang_embed.weight'].double())
    got = ofs2.esm(sd, 'fs2.esm.', Eo, LP, 8, RC.F64)
    err = float((got[0] - table[lang[0]]).abs().max())
    print(f'ESM at B = 1 against the table: {err:.2e}')
    assert err <= 1e-12
    assert float((table[0] - table[1]).abs().max()) > 0.1      # (the two rows differ: a gather by a wrong id would show)


@pytest.mark.parametrize('c', RC.GPU_CASES + [RC.SMALL_GEMM] + RC.LEAK, ids=lambda c: c.name)
def test_cases_tell_the_padded_front_from_the_utterance_alone(c):
    """For every padded row the padded-batch restatement — with the ESM ALREADY per row, so that only the convolutions' padding leak is
    left — differs from the alone oracle by at least 100 x the GPU bound on enc_out, mel_out and pitch_pred; a row without padding agrees."""
    _, hp, sd = RC.model(c.front, c.depth)
    t, a64, _ = ref(c)
    pad = RC.padded_esm_per_row(sd, hp, c, t, RC.F64)
    for k in ('enc_out', 'mel_out', 'pitch_pred'):
        if k not in a64:
            continue
        scale = max(1.0, float(a64[k].abs().max()))
        for b in range(c.B):
            n, full = (c.n_tok[b], c.Tt) if k == 'enc_out' else (c.n_frames[b], c.T)
            d = float((pad[k][b, :n] - a64[k][b, :n]).abs().max()) / scale
            print(f'  {k} row {b} ({n} of {full}): {d:.2e} = {d / RC.BOUND[k]:.0f} x the bound')
            if n < full or (k != 'enc_out' and c.n_tok[b] < c.Tt):
                assert d >= 100 * RC.BOUND[k], (k, b, d)
            else:
                assert d <= 1e-12, (k, b, d)


def test_bounds_cover_the_float32_alone_oracle():
    """BOUND is 4 x the float32 alone oracle's deviation from float64: every case's figures again, each held to bound / 4."""
    worst = {}
    for c in RC.CPU_CASES:
        t, a64, a32 = ref(c)
        for k, v in RC.figures(a32, a64).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if c.mode == 'pred':
            _, hp, sd = RC.model(c.front, c.depth)
            p64, p32 = RC.alone(sd, hp, c, t, RC.F64, predict=True), RC.alone(sd, hp, c, t, RC.F32, predict=True)
            assert torch.equal(p64['dur_choice'], p32['dur_choice']) and int(p64['dur_choice'].sum(-1).min()) > 0
            worst['dur'] = max(worst.get('dur', 0.0), RC.figures(p32, p64)['dur'])
    print({k: f'{v:.3e} (bound / 4 = {RC.MEASURED_F32[k]:.3e})' for k, v in worst.items()})
    assert set(worst) == set(RC.MEASURED_F32)
    for k, v in worst.items():
        assert v <= RC.MEASURED_F32[k], (k, v)


def test_alone_is_zero_beyond_a_row_and_bin_one():
    c = RC.EDGE[0]
    _, a64, _ = ref(c)
    for b in range(c.B):
        assert not a64['enc_out'][b, c.n_tok[b]:].any() and not a64['mel_out'][b, c.n_frames[b]:].any()
        assert bool((a64['pitch_bin'][b, c.n_frames[b]:] == 1).all()) and a64['enc_out'][b, :c.n_tok[b]].abs().max() > 0


def test_lengths_in_one_read_and_the_rows_that_have_none():
    from bisinger_amd.fs2 import prefix_lengths
    txt = torch.tensor([[5, 6, 7, 0], [9, 0, 0, 0], [3, 4, 5, 6]])
    m2p = torch.tensor([[1, 1, 2, 3, 3, 0], [0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 4, 4]])
    assert prefix_lengths([txt > 0, m2p > 0], ['txt_tokens', 'mel2ph'], [1, 0]) == [[3, 1, 4], [5, 0, 6]]
    hole = txt.clone()
    hole[2, 1] = 0
    with pytest.raises(ValueError, match='row 2 of txt_tokens'):
        prefix_lengths([hole > 0], ['txt_tokens'], [1])
    with pytest.raises(ValueError, match='row 1 of txt_tokens'):      # no token at all: n_tok >= 1 is required
        prefix_lengths([torch.tensor([[1, 2], [0, 0]]) > 0], ['txt_tokens'], [1])
    late = m2p.clone()
    late[0, 0] = 0
    with pytest.raises(ValueError, match='row 0 of mel2ph'):
        prefix_lengths([txt > 0, late > 0], ['txt_tokens', 'mel2ph'], [1, 0])


def test_refusals_that_need_no_device():
    """rows= with a ragged switch: NotImplementedError before any model runs; a null handle: BSG_EINVAL with a message."""
    from bisinger_amd.diffusion import GaussianDiffusion
    m, _, _ = RC.model('plain', 2)
    txt = torch.tensor([[5, 6, 0]])
    with pytest.raises(NotImplementedError, match=r'ragged=True, rows='):
        m(txt, torch.tensor([[1, 2, 0]]), None, infer=True, ragged=True, rows=slice(0, 1))
    gd = object.__new__(GaussianDiffusion)
    with pytest.raises(NotImplementedError, match=r'ragged_front=True, rows='):
        GaussianDiffusion.forward(gd, txt, infer=True, ragged_front=True, rows=slice(0, 1))
    with pytest.raises(NotImplementedError, match=r'ragged=True, rows='):      # the pinned refusal stays as it was
        GaussianDiffusion.forward(gd, txt, infer=True, ragged=True, rows=slice(0, 1))
    lib = _lib.load()
    assert lib.bsg_fs2midi_encode_ragged(*([None] * 8), 1, 1, *([None] * 4)) == -22 and 'null argument' in lib.bsg_last_error().decode()
    assert lib.bsg_fs2_encode_plain_ragged(*([None] * 4), 1, 1, *([None] * 4)) == -22 and 'null argument' in lib.bsg_last_error().decode()
    assert lib.bsg_fs2_decode_ragged(*([None] * 9), 1, 1, 1, *([None] * 6)) == -22 and 'null argument' in lib.bsg_last_error().decode()


def test_abi_v20_entries_match_the_header():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'bisinger_hip.h')).read(), flags=re.S)
    assert _lib.ABI_VERSION >= 20 and re.search(rf'#define BSG_ABI_VERSION {_lib.ABI_VERSION}\b', src)      # (v21 added bsg_gemm_h2w_ex)
    for name in ('bsg_fs2midi_encode_ragged', 'bsg_fs2_encode_plain_ragged', 'bsg_fs2_decode_ragged'):
        args = re.search(rf'\bint {name}\s*\((.*?)\);', src, flags=re.S).group(1).split(',')
        restype, argtypes = _lib._SIGS[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, ty in zip(args, argtypes):
            assert ('*' in a) == (ty is _lib.c_void_p), (name, a.strip())
        assert name in _lib.declared_symbols()

