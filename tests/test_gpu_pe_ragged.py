"""GPU: ragged batches through the pitch extractor (bsg_pitchext_forward_ragged, PitchExtractor.forward(lengths=),
forward_batch(ragged_pitch=True)), on both pipes of its GEMMs.

A ragged forward runs the launches of the padded call at (B, T); every launch bounds row b by lengths[b].  What is checked:

  1. every row against the float64 oracle run on THAT ROW ALONE (mel[b:b+1, :n_b]; never the padded oracle, which on rows 1-3 is more
     than 1000 bars away: tests/test_pe_ragged_cpu.py), by _check_pitch of tests/test_gpu_f2_fullsize.py with its own bars.  The mel
     beyond each row's end is NaN and the workspace is filled with NaN bytes first: pitch_pred and f0 must be exactly 0 there, and no
     range event may fire;
  2. every row equals the row-alone call (B = 1, T = n_b) bit for bit: at the three cases (every product on the 64-row forms on both
     sides) and at B = 48, T = 1000, where the batch runs the 128-row forms of both pipes and the row alone the 64-row ones;
  3. all lengths = T is the padded call bit for bit;
  4. a row's result does not change when the other rows and their lengths do;
  5. a short ragged call after a long padded one, on a poisoned workspace, equals a fresh handle's;
  6. a captured ragged forward replays its lengths after the host array has changed;
  7. refusals write nothing;
  8. forward_batch(ragged_pitch=True) end to end on the NSF + pe_enable set-up.
"""
import ctypes
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import yaml

from bisinger_amd import _lib, synth
from tests import pe_cases, pe_ragged_cases as rc
from tests.test_gpu_f2_fullsize import _check_pitch, pitch_ext  # noqa: F401  (the fixture)
from tests.test_gpu_infer import _item, workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)
from tests.test_gpu_pe_shapes import _same, pe_on  # noqa: F401  (pe_on: the extractor on each pipe)
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

KEYS = ('pitch_pred', 'f0_denorm_pred')


def _row(r, b, n):
    return {k: r[k][b:b + 1, :n] for k in KEYS}


def _zero_beyond(r, lens):
    return all(not r[k][b, n:].any() for k in KEYS for b, n in enumerate(lens))


def _ragged_c(pe, mel, lens, pred, f0):
    """bsg_pitchext_forward_ragged itself (no range guard around it): rc."""
    B, T, _ = mel.shape
    arr = lens if lens is None or isinstance(lens, ctypes.Array) else (ctypes.c_int32 * len(lens))(*lens)
    return _lib.load().bsg_pitchext_forward_ragged(pe.handle(), _lib.ptr(mel), arr, _lib.ptr(pred), _lib.ptr(f0), B, T, _lib.stream_ptr())


# ------------------------------------------------------------------------------------------------------------------
# 1. every row alone, against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,lens', rc.CASES, ids=rc.IDS)
def test_rows_alone_vs_fp64(T, lens, pe_on):  # noqa: F811
    pe, sd = pe_on
    m = rc.mel(T, lens)
    pe(torch.from_numpy(m).cuda())                       # (the handle and its workspace exist: the poison below has something to fill)
    retries = _lib.range_retries
    pe.poison_workspace()
    r = pe(torch.from_numpy(rc.nan_tail(m, lens)).cuda(), lengths=lens)
    assert r['pitch_pred'].shape == (rc.B, T, 2) and r['f0_denorm_pred'].shape == (rc.B, T)
    assert all(torch.isfinite(r[k]).all() for k in KEYS)
    for b, n in enumerate(lens):
        _check_pitch(f'pitch_extractor ragged T={T} row {b} n={n}', _row(r, b, n), sd, m[b:b + 1, :n].copy(), [n])
    assert _zero_beyond(r, lens), 'pitch_pred / f0 beyond a row\'s end are not 0'
    assert _lib.range_retries == retries, 'a NaN tail raised a range event of the split-fp16 GEMMs'
    assert pe.gemm_range_peek() == 0 and _lib.gemm_range_peek() == 0


# ------------------------------------------------------------------------------------------------------------------
# 2. every row alone, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,lens', rc.CASES, ids=rc.IDS)
def test_rows_equal_the_row_alone_call_bitwise(T, lens, pe_on):  # noqa: F811
    pe, _ = pe_on
    m = rc.mel(T, lens)
    r = pe(torch.from_numpy(rc.nan_tail(m, lens)).cuda(), lengths=torch.tensor(lens))
    for b, n in enumerate(lens):
        alone = pe(torch.from_numpy(m[b:b + 1, :n].copy()).cuda())
        assert _same(_row(r, b, n), alone), f'row {b} (n={n})'


def test_rows_on_the_128_row_forms_bitwise(pe_on):  # noqa: F811
    """B = 48, T = 1000: 2 x 8 x 48 = 768 workgroups of 128 rows, the count from which both pipes take their 128-row forms (fp32 from 512,
    split-fp16 from 768); a row alone takes the 64-row ones.  An element's sum order depends on neither the tile height nor the tile's
    place, so the rows still agree bit for bit.  Row ends on, before and after the 128-row seams, and one frame."""
    pe, _ = pe_on
    B, T = 48, 1000
    rs = np.random.RandomState(48)
    lens = [1000, 897, 896, 895, 129, 128, 127, 1] + rs.randint(2, T, size=B - 8).tolist()
    mel = torch.from_numpy((rs.standard_normal((B, T, 80)) * 1.5 - 3.0).astype(np.float32)).cuda()
    ragged_in = mel.clone()
    for b, n in enumerate(lens):
        ragged_in[b, n:] = float('nan')
    retries = _lib.range_retries
    r = pe(ragged_in, lengths=lens)
    assert _zero_beyond(r, lens)
    for b in (0, 1, 2, 3, 4, 5, 6, 7, 20, 47):
        n = lens[b]
        assert _same(_row(r, b, n), pe(mel[b:b + 1, :n].contiguous())), f'row {b} (n={n})'
    assert _lib.range_retries == retries and pe.gemm_range_peek() == 0


# ------------------------------------------------------------------------------------------------------------------
# 3. all lengths = T is the padded call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', [(3, 129), (1, 5), (3, 65)])
def test_full_lengths_are_the_padded_call(B, T, pe_on):  # noqa: F811
    pe, _ = pe_on
    mel = torch.from_numpy(pe_cases.mel_for(B, T)).cuda()
    want = pe(mel)
    pe.poison_workspace()
    got = pe(mel, lengths=[T] * B)
    assert _same(got, want)


# ------------------------------------------------------------------------------------------------------------------
# 4. rows do not see each other
# ------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_itself_alone(pe_on):  # noqa: F811
    pe, _ = pe_on
    T, lens = rc.CASES[0]
    m = rc.mel(T, lens)
    a = pe(torch.from_numpy(rc.nan_tail(m, lens)).cuda(), lengths=lens)
    other_lens = [12, lens[1], 129, lens[3]]
    other = rc.mel(T + 1, [T + 1] * rc.B)[:, :T].copy()
    other[1], other[3] = m[1], m[3]
    b = pe(torch.from_numpy(rc.nan_tail(other, other_lens)).cuda(), lengths=other_lens)
    assert _same(_row(a, 1, lens[1]), _row(b, 1, lens[1]))
    assert not torch.equal(a['pitch_pred'][0, :12], b['pitch_pred'][0, :12])


# ------------------------------------------------------------------------------------------------------------------
# 5. workspace reuse
# ------------------------------------------------------------------------------------------------------------------
def test_short_ragged_after_long_padded_equals_fresh_handle(pe_on, sd_spec):  # noqa: F811
    pe, _ = pe_on
    fresh = pe_cases.pitch_extractor(sd_spec).cuda()
    fresh.set_gemm_split(pe.gemm_split_enabled())
    pe(torch.from_numpy(pe_cases.mel_for(3, 257)).cuda())
    pe.poison_workspace()
    T, lens = rc.CASES[1]
    mel = torch.from_numpy(rc.nan_tail(rc.mel(T, lens), lens)).cuda()
    got = pe(mel, lengths=lens)
    want = fresh(mel, lengths=lens)
    fresh.release()
    assert all(torch.isfinite(got[k]).all() for k in KEYS)
    assert _same(got, want)


# ------------------------------------------------------------------------------------------------------------------
# 6. capture
# ------------------------------------------------------------------------------------------------------------------
def test_captured_ragged_forward_replays_its_lengths(pe_on):  # noqa: F811
    pe, _ = pe_on
    T, lens = rc.CASES[0]
    mel = torch.from_numpy(rc.nan_tail(rc.mel(T, lens), lens)).cuda()
    eager = pe(mel, lengths=lens)
    arr = (ctypes.c_int32 * rc.B)(*lens)
    pred, f0 = torch.empty(rc.B, T, 2, device='cuda'), torch.empty(rc.B, T, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(_ragged_c(pe, mel, arr, pred, f0), 'warm-up')
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(_ragged_c(pe, mel, arr, pred, f0), 'capture')
    for i in range(rc.B):
        arr[i] = 1                  # the host array is read before the call returns: the replay keeps the captured counts
    pe.poison_workspace()
    pred.fill_(float('nan'))
    f0.fill_(float('nan'))
    g.replay()
    torch.cuda.synchronize()
    assert pe.gemm_range_peek() == 0
    assert _same({'pitch_pred': pred, 'f0_denorm_pred': f0}, eager)


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(pe_on):  # noqa: F811
    pe, _ = pe_on
    B, T = 2, 5
    mel = torch.from_numpy(pe_cases.mel_for(B, T)).cuda()
    pe(mel)
    lib = _lib.load()
    for lens, row in (([5, 0], 1), ([6, 5], 0), ([5, -3], 1)):
        pred, f0 = torch.full((B, T, 2), 7.0, device='cuda'), torch.full((B, T), 7.0, device='cuda')
        rc_ = _ragged_c(pe, mel, lens, pred, f0)
        torch.cuda.synchronize()
        assert rc_ == -22, (lens, rc_)
        msg = lib.bsg_last_error().decode()
        assert f'lengths[{row}]={lens[row]}' in msg and f'1..T={T}' in msg, msg
        assert bool((pred == 7.0).all()) and bool((f0 == 7.0).all()), lens
        with pytest.raises(_lib.BsgError, match=rf'lengths\[{row}\]={lens[row]} outside 1\.\.T={T}'):
            pe(mel, lengths=lens)
    pred, f0 = torch.full((B, T, 2), 7.0, device='cuda'), torch.full((B, T), 7.0, device='cuda')
    assert _ragged_c(pe, mel, None, pred, f0) == -22 and 'lengths_host is null' in lib.bsg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((pred == 7.0).all()) and bool((f0 == 7.0).all())
    with pytest.raises(_lib.BsgError, match='lengths has 3 entries for a batch of 2 rows'):
        pe(mel, lengths=[5, 5, 5])
    assert _same(pe(mel, lengths=torch.tensor([5, 5])), pe(mel))      # the handle is as usable as before


# ------------------------------------------------------------------------------------------------------------------
# 8. end to end
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def nsf_workdir(workdir, sd_spec):  # noqa: F811
    """The pe_enable + use_nsf set-up of tests/test_gpu_infer.py (exp2.yaml in the synthetic checkpoint directory)."""
    os.makedirs('checkpoints/pe')
    os.makedirs('checkpoints/nsf')
    spec = OrderedDict((k, tuple(s)) for k, s in sd_spec['PitchExtractor'])
    pw = synth.synth_state_dict(spec, seed=11)
    for k in spec:
        if k.endswith('running_var'):
            pw[k] = (0.5 + np.abs(pw[k]) * 5).astype(np.float32)
    pe_sd = {k: torch.from_numpy(v) for k, v in pw.items()}
    for k, s_ in spec.items():
        if k not in pe_sd:
            pe_sd[k] = torch.zeros(s_, dtype=torch.long if k.endswith('num_batches_tracked') else torch.float32)
    torch.save({'state_dict': {'model.' + k: v for k, v in pe_sd.items()}}, 'checkpoints/pe/model_ckpt_steps_10.ckpt')
    nspec = OrderedDict((k, tuple(s)) for k, s in sd_spec['HifiGanGenerator_nsf_weight_norm'])
    nsd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(nspec, seed=13).items()}
    torch.save({'state_dict': {'model_gen': nsd}}, 'checkpoints/nsf/model_ckpt_steps_7.ckpt')
    hcfg = yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml'))
    hcfg['use_pitch_embed'] = True
    yaml.safe_dump(hcfg, open('checkpoints/nsf/config.yaml', 'w'))
    cfg = yaml.safe_load(open('exp.yaml'))
    cfg.update(vocoder_ckpt='checkpoints/nsf', pe_enable=True, pe_ckpt='checkpoints/pe', use_nsf=True, pitch_type='frame', use_uv=True,
               pitch_norm='log')
    yaml.safe_dump(cfg, open('exp2.yaml', 'w'))
    return workdir


def test_forward_batch_ragged_pitch(nsf_workdir):
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp2.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=99')
    infer = DiffSingerE2EInfer(hparams)
    assert infer.vocoder.use_nsf and hasattr(infer, 'pe')
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3), (4, 4), (7, 5))]
    pe = infer.pe
    sd = pe_cases.cpu_state_dict(pe)
    calls = []
    inner = pe.forward

    def recording(mel, *a, **kw):
        out = inner(mel, *a, **kw)
        calls.append((mel.clone(), kw.get('lengths'), out))
        return out
    pe.forward = recording
    before = _lib.range_retries
    kw = dict(seed=77, max_sentences=3, ragged=True, ragged_vocoder=True)
    wavs = infer.forward_batch(items, ragged_pitch=True, **kw)
    st = infer.last_batch_stats
    ragged_calls, calls[:] = list(calls), []
    today = infer.forward_batch(items, **kw)
    explicit = infer.forward_batch(items, ragged_pitch=False, **kw)
    padded_calls = list(calls)
    pe.forward = inner
    assert len(ragged_calls) == len(st['buckets']) == 2 and len(padded_calls) == 4
    assert all(c[1] is None for c in padded_calls)
    for i in range(len(items)):
        assert wavs[i].shape == today[i].shape and np.isfinite(wavs[i]).all()
        assert np.array_equal(explicit[i], today[i])      # the default is the padded extractor, given as a keyword or not
    moved = False
    for bk, (mel, lens, out), (pmel, _, pout) in zip(st['buckets'], ragged_calls, padded_calls):
        assert list(lens) == [st['frames'][i] for i in bk]
        assert torch.equal(mel, pmel)                       # same mel: the keyword changes the extractor's call only
        for r, i in enumerate(bk):
            n = st['frames'][i]
            row = mel[r:r + 1, :n].contiguous()
            alone = pe(row)
            # _check_pitch's rule with the row-alone call of the same extractor as the target: pitch_pred within the bar, the voicing
            # wherever the logit is clear of 0 by 10 bars, f0 within 2^bar - 1 there
            bar = pe_cases.oracle_margin(sd, row.cpu().numpy())[0]
            pp, pp_alone = out['pitch_pred'][r, :n].double().cpu().numpy(), alone['pitch_pred'][0].double().cpu().numpy()
            f0, f0_alone = out['f0_denorm_pred'][r, :n].double().cpu().numpy(), alone['f0_denorm_pred'][0].double().cpu().numpy()
            assert np.abs(pp - pp_alone).max() <= bar, (i, n)
            clear = np.abs(pp_alone[:, 1]) > 10 * bar
            assert ((f0 > 0) == (f0_alone > 0))[clear].all()
            voiced = clear & (f0_alone > 0)
            assert (np.abs(f0 - f0_alone)[voiced] <= (2 ** bar - 1 + 1e-6) * f0_alone[voiced]).all()
            assert not out['f0_denorm_pred'][r, n:].any()
            if n < mel.shape[1]:
                moved |= not torch.equal(out['f0_denorm_pred'][r, :n], pout['f0_denorm_pred'][r, :n])
    assert moved, 'no shorter row got another f0 than the padded extractor gives it'
    assert _lib.range_retries == before and pe.gemm_range_peek() == 0
    hparams['pe_enable'] = False
    try:
        with pytest.raises(ValueError, match='pe_enable'):
            infer.forward_batch(items, seed=77, max_sentences=3, ragged_pitch=True)
    finally:
        hparams['pe_enable'] = True
