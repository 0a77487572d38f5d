"""GPU: the frame-level pitch adaptor (use_pitch_embed) and the plain FastSpeech2 front, through the C ABI (bsg_fs2_create,
bsg_fs2_encode_plain, bsg_fs2_decode), against the float64 restatement of tests/fs2_pitch_ref.py.

Bounds: fs2_pitch_ref.BOUND, one per output — 4 x the float32 restatement's own deviation from float64 (measured on the CPU, held by
tests/test_fs2_pitch_cpu.py), x max(1, max |want|); f0_denorm relative to max(1, f0).  Bins are exact except at near ties (a frame whose
float64 f0_mel + 0.5 lies within TIE_DELTA of an integer, or whose |pitch_pred[..., 1]| is inside the bound): there either neighbour, or
either uv state, is accepted with its decoder_inp row, and such frames may be at most 2 % of a case's real frames.  With predicted f0 the
check has two stages: pitch_pred and f0_denorm against float64; everything downstream against the float64 restatement FED the GPU's own
pitch_pred (f0 = pred[..., 0], uv = pred[..., 1] > 0), so that one flipped bin is not spread through the decoder's attention.
"""
import json
import os

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import fs2_pitch_ref as R
from tests.util import ROOT, cpu_sd

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64 = torch.float64
_MODELS = {}
_GOLD_MODELS = {}     # test_goldens: models that index the position tables of the host that made the goldens


def model(front, depth=2, use_uv=True, spk=None, pitch=True):
    key = (front, depth, use_uv, spk, pitch)
    if key not in _MODELS:
        m, hp = R.build(front, depth, use_uv, spk, pitch=pitch)
        _MODELS[key] = (m.cuda(), hp, cpu_sd(m, 'fs2.'))
    return _MODELS[key]


def pit_tokens(L):
    """The adaptor's launch record for an L-layer predictor: the aligned 256-channel convolutions can only take the split-fp16 form with
    64-row tiles under the guard; a form launched in every layer is named once, and pit.launches counts what was launched: the position
    scan, the entry, L convolutions, L - 1 LayerNorms, the tail."""
    return ['pit.pos', 'pit.entry', 'pit.gemm:gemm_split/64'] + (['pit.ln'] if L > 1 else []) + ['pit.tail', f'pit.launches:{2 * L + 2}']


def dev(inp):
    return {k: torch.from_numpy(v).cuda() for k, v in inp.items()}


def rel(got, want):
    want = want.double()
    d = float((got.detach().cpu().double() - want).abs().max())
    print(f'    max-abs {d:.3e}  max |want| {float(want.abs().max()):.3e}')
    return d / max(1.0, float(want.abs().max()))


def check_pitch(got, r64, real, mode, use_uv, what, f0_given=None):
    """Stage 1 (pitch_pred, f0_denorm within the bounds) and the bins with the near-tie rule (bin ties where f0 is predicted, uv ties where uv
    is); -> the near-tie mask."""
    print(f'  {what}')
    assert rel(got['pitch_pred'], r64['pitch_pred']) <= R.BOUND['pitch_pred']
    tie, uv_tie = R.near_ties(r64)
    tie = tie if mode == 'pred' else torch.zeros_like(real)
    uv_tie = uv_tie if (mode != 'f0uv' and use_uv) else torch.zeros_like(real)
    loose = (tie | uv_tie) & real
    assert float(loose.sum()) <= 0.02 * float(real.sum()), 'near ties above 2 % of the real frames'
    f0g, f0w = got['f0_denorm'].cpu().double(), r64['f0_denorm'].double()
    fr = ((f0g - f0w).abs() / f0w.clamp(min=1))[~loose]
    print(f'    f0_denorm rel {float(fr.max()) if fr.numel() else 0.0:.3e}  near ties {int(loose.sum())} of {int(real.sum())}')
    assert fr.numel() == 0 or float(fr.max()) <= R.BOUND['f0_denorm']
    bg, bw = got['pitch_bin'].cpu(), r64['pitch_bin']
    assert torch.equal(bg[~loose], bw[~loose]), 'bins differ away from a near tie'
    assert bool(((bg - bw).abs()[loose & ~uv_tie] <= 1).all()), 'a near tie took a bin that is no neighbour'
    if mode == 'f0':     # supplied f0, predicted uv: at a uv tie the bin is the supplied f0's or the unvoiced one, nothing else
        voiced = R.f0_to_mel_bins(2 ** f0_given.double())[1]
        at = loose & uv_tie
        assert bool(((bg == voiced) | (bg == 1))[at].all()), 'a uv tie took a bin that is neither the supplied f0\'s nor 1'
    assert bool((got['f0_denorm'].cpu()[~real] == 0).all()) and bool((bg[~real] == 1).all())
    return loose


def check_decoder_inp(got, r64, sd, real):
    """decoder_inp against the restatement's, every frame: where the GPU took the other bin of a near tie (check_pitch allowed it), the
    restatement's row is moved to that bin's pitch_embed row — the matching row."""
    E = sd['fs2.pitch_embed.weight'].double()
    bg, bw = got['pitch_bin'].cpu(), r64['pitch_bin']
    dw = r64['decoder_inp'].double() + (E[bg] - E[bw]) * real[..., None]
    dg = got['decoder_inp'].cpu().double()
    err = float((dg - dw).abs().max()) / max(1.0, float(dw.abs().max()))
    print(f'  decoder_inp {err:.3e} (x max(1, max |want|))')
    assert err <= R.BOUND['decoder_inp']
    assert bool((dg[~real] == 0).all())


@pytest.mark.parametrize('case', R.frame_cases(), ids=lambda c: f'{c[0]}-L{c[1]}-uv{int(c[2])}-{c[3]}-{c[4]}x{c[5]}')
def test_predictor_and_tail_at_shape_edges(case):
    front, depth, use_uv, mode, B, T, lens = case
    m, hp, sd = model(front, depth, use_uv)
    Tt = max(1, min(12, T // 3 + 1))
    inp = R.frame_inputs(B, Tt, T, lens)
    d = dev(inp)
    f0 = d['f0'] if mode in ('f0', 'f0uv') else None
    uv = d['uv'] if mode == 'f0uv' else None
    f0_keep = None if f0 is None else f0.clone()
    got = m.decode_all(d['enc_out'], d['mel2ph'], d['spk_embed'] if hp['use_spk_id'] else None,
                       d['speechsing'] if hp['use_midi'] else None, skip_decoder=True, f0=f0, uv=uv)
    assert m.gemm_range_take() == 0
    assert m.last_path().split() == pit_tokens(depth), m.last_path()      # decode only: nothing but the adaptor's launches
    if f0 is not None:
        assert torch.equal(f0, f0_keep), "the caller's f0 was written"
    r64 = R.frame_reference(sd, hp, inp, mode, F64)
    real = torch.from_numpy(inp['mel2ph']) > 0
    check_pitch(got, r64, real, mode, use_uv, 'against float64', f0_given=None if f0 is None else f0.cpu())
    if mode == 'pred':
        # stage 2: downstream of the GPU's own prediction (uv = pred[..., 1] > 0 is then the GPU's own decision: only bin ties remain)
        fed = dict(inp, f0=got['pitch_pred'][..., 0].cpu().numpy(), uv=(got['pitch_pred'][..., 1] > 0).float().cpu().numpy())
        r64 = R.frame_reference(sd, hp, fed, 'f0uv', F64)
        tie = R.near_ties(r64)[0] & real
        bg, bw = got['pitch_bin'].cpu(), r64['pitch_bin']
        assert torch.equal(bg[~tie], bw[~tie]) and bool(((bg - bw).abs()[tie] <= 1).all())
    check_decoder_inp(got, r64, sd, real)


PLAIN = [(1, 1, 3, None, False), (2, 2, 7, (2, 1), True), (2, 31, 70, (31, 17), False), (3, 32, 65, (32, 5, 32), True), (2, 33, 64, (33, 30), False),
         (2, 100, 203, (100, 41), True)]


def _plain_inputs(B, Tt, T, lens):
    inp = synth.synth_inputs(B, Tt, T, seed=5, num_spk=2)
    rs = np.random.RandomState(B * 1000 + Tt)
    if lens:
        for b, n in enumerate(lens):
            inp['txt_tokens'][b, n:] = 0
            inp['mel2ph'][b] = np.minimum(np.arange(T) * Tt // T + 1, n)
            inp['mel2ph'][b, T * n // Tt:] = 0
        if Tt >= 31:
            inp['txt_tokens'][0, 3] = 0          # a padded token INSIDE a row: positions count the non-pad tokens only
            inp['mel2ph'][0][inp['mel2ph'][0] == 4] = 3
    inp['f0'] = R.bin_centre_f0(rs.randint(2, 255, size=(B, T)))
    inp['uv'] = (rs.uniform(size=(B, T)) < 0.2).astype(np.float32)
    return inp


@pytest.mark.parametrize('B,Tt,T,lens,spk', PLAIN, ids=lambda v: str(v).replace(' ', ''))
def test_plain_front(B, Tt, T, lens, spk):
    m, hp, sd = model('plain', 2, True, spk)
    inp = _plain_inputs(B, Tt, T, lens)
    d = dev(inp)
    ti = {k: torch.from_numpy(v) for k, v in inp.items()}
    got = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'] if spk else None, f0=d['f0'], uv=d['uv'], infer=True)
    path = m.last_path().split()
    assert path[0] == 'tok:front' and [t for t in path if t.startswith('pit.')] == pit_tokens(2), path
    assert all(t.split('.')[0] in ('tok:front', 'enc', 'pit', 'dec') for t in path), path
    assert path.index('pit.pos') > max(i for i, t in enumerate(path) if t.startswith('enc.')) and path.index('pit.launches:6') < path.index(
        next(t for t in path if t.startswith('dec.'))), path
    assert m.gemm_range_take() == 0
    r64 = R.forward(sd, ti, hp, dtype=F64, f0=ti['f0'], uv=ti['uv'])
    enc = m.encode(d['txt_tokens'], d['spk_embed'] if spk else None)['enc_out']
    assert rel(enc, r64['enc_out']) <= R.BOUND['enc_out']
    assert torch.equal(got['pitch_bin'].cpu(), r64['pitch_bin'])
    assert rel(got['pitch_pred'], r64['pitch_pred']) <= R.BOUND['pitch_pred']
    assert rel(got['decoder_inp'], r64['decoder_inp']) <= R.BOUND['decoder_inp']
    assert rel(got['mel_out'], r64['mel_out']) <= R.BOUND['mel_out']
    # rows: the plain front has no cross-row coupling
    if B > 1:
        part = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'] if spk else None, f0=d['f0'], uv=d['uv'], infer=True, rows=slice(1, B))
        assert m.last_rows()[0] == (B - 1) * Tt
        # (not bit for bit: launch_gemm and the stacks pick their tile heights by the rows of the call, another order of the same sums, as
        # tests/test_gpu_fs2.py::test_fs2_rank_rows_front notes for the MIDI front)
        dr = float((part['mel_out'] - got['mel_out'][1:]).abs().max())
        print(f'    rows 1:{B} against the whole batch: {dr:.3e}')
        assert dr <= 1e-5 and torch.equal(part['pitch_bin'], got['pitch_bin'][1:])
    # predicted durations: the integer outputs are exact
    pred = m(d['txt_tokens'], None, d['spk_embed'] if spk else None, infer=True, skip_decoder=True)
    want = R.forward(sd, {k: v for k, v in ti.items() if k != 'mel2ph'}, hp, dtype=F64, skip_decoder=True)
    assert torch.equal(pred['mel2ph'].cpu(), want['mel2ph'])


def test_midi_with_adaptor_end_to_end_predicted_f0():
    """FastSpeech2MIDI + use_pitch_embed, predicted f0, B = 2, T_txt = 12, T = 64 with a padded row: the two stages of the module docstring."""
    m, hp, sd = model('midi', 5, True)
    inp = synth.synth_inputs(2, 12, 64, seed=1, ragged=True)
    d = dev(inp)
    ti = {k: torch.from_numpy(v) for k, v in inp.items()}
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    got = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], infer=True, **kw)
    r64 = R.forward(sd, ti, hp, dtype=F64)
    real = ti['mel2ph'] > 0
    check_pitch(got, r64, real, 'pred', True, 'against float64')
    fed = R.forward(sd, ti, hp, dtype=F64, f0=got['pitch_pred'][..., 0].cpu(), uv=(got['pitch_pred'][..., 1] > 0).float().cpu())
    assert torch.equal(got['pitch_bin'].cpu(), fed['pitch_bin'])
    assert rel(got['decoder_inp'], fed['decoder_inp']) <= R.BOUND['decoder_inp']
    assert rel(got['mel_out'], fed['mel_out']) <= R.BOUND['mel_out']
    assert got['f0_denorm'].shape == (2, 64) and got['pitch_pred'].shape == (2, 64, 2)


def test_short_call_after_long_one_on_poisoned_workspace_and_capture():
    m, hp, sd = model('plain', 2, True)
    long_inp, short_inp = _plain_inputs(2, 100, 203, (100, 41)), _plain_inputs(2, 31, 70, (31, 17))

    def run(mod, inp, f0=True):
        d = dev(inp)
        return mod(d['txt_tokens'], d['mel2ph'], None, f0=d['f0'] if f0 else None, uv=d['uv'] if f0 else None, infer=True)
    run(m, long_inp)
    m.poison_workspace()
    a = run(m, short_inp, f0=False)
    fresh, _ = R.build('plain', 2, True)
    fresh = fresh.cuda()
    b = run(fresh, short_inp, f0=False)
    for k in ('pitch_pred', 'f0_denorm', 'pitch_bin', 'decoder_inp', 'mel_out'):
        assert torch.equal(a[k], b[k]), k
    # a captured replay is bit-identical to eager
    d = dev(short_inp)
    enc = m.encode(d['txt_tokens'], None)['enc_out']
    eager = m.decode_all(enc, d['mel2ph'], None, None)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.decode_all(enc, d['mel2ph'], None, None)       # warm-up on the side stream (workspaces are sized)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = m.decode_all(enc, d['mel2ph'], None, None)
    for v in cap.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k], cap[k]), k


def test_midi_handle_without_pitch_matches_the_old_create_path():
    """bsg_fs2_create with front MIDI and use_pitch_embed 0 against bsg_fs2midi_create (same build, old entry points): bit-identical."""
    from ctypes import POINTER, byref, c_void_p, cast
    m, hp, sd = model('midi', 2, True, pitch=False)
    inp = synth.synth_inputs(2, 12, 64, seed=1, ragged=True)
    d = dev(inp)
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    old = m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], infer=True, **kw)          # bsg_fs2midi_create / _encode / _decode
    assert 'pitch_pred' not in old
    lib = _lib.load()
    ws = [p.detach() for p in m._weights()]
    base = _lib.Fs2Cfg(256, 65, 4, 4, 2, 9, 9, 80, len(m.dur_predictor.conv), m.dur_predictor.kernel_size, m.spk_embed_proj.num_embeddings, 8,
                       m._n_pos, m._n_rel)
    cfg = _lib.Fs2XCfg(base, _lib.FS2_FRONT_MIDI, 0, 0, 0, 0, 0)
    assert lib.bsg_fs2_n_weights(byref(cfg)) == len(ws) == 143
    dec_table = m.decoder.embed_positions.table(m._n_pos).cuda().contiguous()
    tok_table = m._token_table().cuda().contiguous()
    arr = (c_void_p * len(ws))(*[p.data_ptr() for p in ws])
    h = c_void_p()
    _lib.check(lib.bsg_fs2_create(byref(h), byref(cfg), cast(arr, POINTER(c_void_p)), len(ws), _lib.ptr(dec_table), _lib.ptr(tok_table), None,
                                  _lib.stream_ptr()), 'bsg_fs2_create')
    try:
        enc = torch.empty(2, 12, 256, device='cuda')
        dinp, mel = torch.empty(2, 64, 256, device='cuda'), torch.empty(2, 64, 80, device='cuda')
        _lib.check(lib.bsg_fs2midi_encode(h, _lib.ptr(d['txt_tokens']), _lib.ptr(d['pitch_midi']), _lib.ptr(d['midi_dur']), _lib.ptr(d['is_slur']),
                                          _lib.ptr(d['lang']), _lib.ptr(d['spk_embed']), 2, 12, _lib.ptr(enc), None, None, _lib.stream_ptr()), 'encode')
        _lib.check(lib.bsg_fs2_decode(h, _lib.ptr(enc), _lib.ptr(d['mel2ph']), _lib.ptr(d['spk_embed']), _lib.ptr(d['speechsing']), None, None, 2, 12,
                                      64, None, None, None, _lib.ptr(dinp), _lib.ptr(mel), _lib.stream_ptr()), 'decode')
        torch.cuda.synchronize()
        assert torch.equal(dinp, old['decoder_inp']) and torch.equal(mel, old['mel_out'])
    finally:
        lib.bsg_fs2midi_destroy(h)


# ----------------------------------------------------------------------------------------------- the reference's own outputs
def _gold_inputs():
    inp = synth.synth_inputs(2, 12, 64, seed=1, ragged=True)
    rs = np.random.RandomState(64)
    inp['f0'] = R.bin_centre_f0(rs.randint(2, 255, size=(2, 64)))
    inp['uv'] = (rs.uniform(size=(2, 64)) < 0.2).astype(np.float32)
    return inp


@pytest.mark.parametrize('chain,run', [('popcs', 'pred'), ('popcs', 'given'), ('popcs', 'dur'), ('bisinger', 'pred'), ('bisinger', 'given')])
def test_goldens(gold, monkeypatch, chain, run):
    """tests/golden/fs2_pitch.npz (tools/make_golden_fs2pitch.py): the reference's FastSpeech2 / FastSpeech2MIDI with use_pitch_embed on the
    formula weights, B = 2, T_txt = 12, T = 64, one row padded in tokens and frames.

    The position tables are host work (float32 exp, sin, cos, in the reference and in the drop-in alike), and the float32 exp of the host
    that made the goldens differs by an ulp here and there from another host's; the MIDI front's reversed table multiplies that ulp by up
    to 4999.  With tables built on the testing host, decoder_inp of the MIDI chain sat 1.07e-5 max-abs from the golden (3.0e-6 x
    max |want|, 2.44e-6 allowed) while being 1.2e-6 from the float64 restatement evaluated on that same host — the difference was the
    tables', not the kernels'.  So the models of this test index the tables of the golden host (tests/golden/inv_freq.npz through the
    oracle's table functions, fs2_pitch_ref.use_golden_host_tables), as tests/test_oracle_golden.py evaluates the oracle.  Bounds unchanged.
    Measured on an MI355X (x max(1, max |want|); allowed pitch_pred 1.40e-6, decoder_inp 2.44e-6, mel_out 3.43e-6): PopCS chain 3.9e-7 / 4.0e-7 /
    1.05e-6, BiSinger chain 4.5e-7 / 8.0e-7 / 8.5e-7."""
    from oracle import freq
    monkeypatch.setattr(freq, 'inv_freq', R.golden_host_inv_freq())
    g = gold('fs2_pitch')
    midi = chain == 'bisinger'
    if chain not in _GOLD_MODELS:
        mm, hp_, = R.build('midi', 5, True) if midi else R.build('plain', 2, True)
        _GOLD_MODELS[chain] = (R.use_golden_host_tables(mm.cuda()), hp_, cpu_sd(mm, 'fs2.'))
    m, hp, sd = _GOLD_MODELS[chain]
    inp = _gold_inputs()
    d = dev(inp)
    kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')} if midi else {}
    f0, uv = (d['f0'], d['uv']) if run == 'given' else (None, None)
    got = m(d['txt_tokens'], None if run == 'dur' else d['mel2ph'], d['spk_embed'] if midi else None, f0=f0, uv=uv, infer=True, **kw)
    w = lambda k: torch.from_numpy(g[f'{chain}.{run}.{k}'])
    assert torch.equal(got['mel2ph'].cpu(), w('mel2ph'))
    assert rel(got['pitch_pred'], w('pitch_pred')) <= R.BOUND['pitch_pred']
    f0g, f0w = got['f0_denorm'].cpu().double(), w('f0_denorm').double()
    bw = R.f0_to_mel_bins(f0w)[1]
    same = (f0g == 0) == (f0w == 0)          # (a predicted uv decision next to 0 may fall either way: checked against float64 elsewhere)
    assert float((~same).double().mean()) <= 0.02
    assert float(((f0g - f0w).abs() / f0w.clamp(min=1))[same].max()) <= R.BOUND['f0_denorm']
    if torch.equal(got['pitch_bin'].cpu(), bw):
        assert rel(got['decoder_inp'], w('decoder_inp')) <= R.BOUND['decoder_inp']
        assert rel(got['mel_out'], w('mel_out')) <= R.BOUND['mel_out']
    else:
        assert run != 'given', 'bins of a supplied bin-centre f0 differ from the reference'
        ti = {k: torch.from_numpy(v) for k, v in inp.items() if not (run == 'dur' and k == 'mel2ph')}
        fed = R.forward(sd, ti, hp, dtype=F64, f0=got['pitch_pred'][..., 0].cpu(), uv=(got['pitch_pred'][..., 1] > 0).float().cpu())
        assert torch.equal(got['pitch_bin'].cpu(), fed['pitch_bin'])
        assert rel(got['mel_out'], fed['mel_out']) <= R.BOUND['mel_out']


def test_gaussian_diffusion_popcs_golden(gold):
    """(c): GaussianDiffusion around the plain front, one shallow K_step = 51 DDPM run of 100 with supplied noise and supplied f0 / uv,
    against the reference's mel.  The 51-step mel is held to the project's bar for sampled mels against reference goldens
    (tests/test_gpu_melgen.py: 1e-3); fs2_mel, the sampler's start, to this file's mel_out bound."""
    from bisinger_amd.diffnet import DiffNet
    from bisinger_amd.diffusion import GaussianDiffusion
    from bisinger_amd.fs2 import FastSpeech2
    from bisinger_amd.hparams import hparams
    from tests.util import load_formula_weights, use_config
    g = gold('fs2_pitch')
    use_config()
    try:
        hparams.update(R.POPCS_HP)
        hparams.update(dilation_cycle_length=1, timesteps=100, K_step=51, max_beta=0.06, gaussian_start=False, pndm_speedup=0)
        with open(os.path.join(ROOT, 'tests', 'golden', 'fs2_pitch_spec.json')) as f:
            rec = json.load(f)['popcs']['hparams']
        hparams.update(spec_min=rec['spec_min'], spec_max=rec['spec_max'], keep_bins=rec['keep_bins'])      # the PopCS chain's own mel range
        del hparams['use_midi']
        gd = GaussianDiffusion(R.PhoneEncoder(), 80, DiffNet(80), timesteps=100, K_step=51, loss_type='l1', spec_min=hparams['spec_min'],
                               spec_max=hparams['spec_max'])
        assert type(gd.fs2) is FastSpeech2
        load_formula_weights(gd, 0, synth.DIFFNET_GAIN)
        with torch.no_grad():
            R.make_pitch_visible({k: v for k, v in gd.state_dict().items()})
        gd = gd.cuda().eval()
        d = dev(_gold_inputs())
        noise = torch.from_numpy(synth.synth_noise(51, 2, 80, 64, seed=3)).cuda()
        f0_keep = d['f0'].clone()
        out = gd(d['txt_tokens'], mel2ph=d['mel2ph'], f0=d['f0'], uv=d['uv'], infer=True, noise=noise)
        assert torch.equal(d['f0'], f0_keep), "the caller's f0 was written"
        assert set(('decoder_inp', 'f0_denorm', 'fs2_mel', 'mel2ph', 'mel_out', 'pitch_pred')) <= set(out)
        assert rel(out['fs2_mel'], torch.from_numpy(g['popcs.gd.fs2_mel'])) <= R.BOUND['mel_out']
        assert rel(out['f0_denorm'], torch.from_numpy(g['popcs.gd.f0_denorm'])) <= R.BOUND['f0_denorm']
        assert float((out['mel_out'].cpu() - torch.from_numpy(g['popcs.gd.mel_out'])).abs().max()) <= 1e-3
        # ragged=True keeps working with the plain front: every row decoded at its own length, mel_out 0 beyond; the full-length row sees
        # the same draws on the same frames as in the padded call
        rag = gd(d['txt_tokens'], mel2ph=d['mel2ph'], f0=d['f0'], uv=d['uv'], infer=True, noise=noise, ragged=True)
        lens = (d['mel2ph'] > 0).sum(-1).tolist()
        assert lens[0] == 64 and lens[1] < 64 and bool(torch.isfinite(rag['mel_out']).all())
        for b, n in enumerate(lens):
            assert bool((rag['mel_out'][b, n:] == 0).all()) and bool((rag['mel_out'][b, :n] != 0).any())
        assert float((rag['mel_out'][0] - out['mel_out'][0]).abs().max()) <= 1e-3
        assert torch.equal(rag['pitch_bin'], out['pitch_bin']) and torch.equal(rag['f0_denorm'], out['f0_denorm'])
    finally:
        use_config()


# ----------------------------------------------------------------------------------------------- the inference harness
from tests.test_gpu_infer import _item, workdir      # noqa: E402,F401  (the synthetic checkpoint directory of the harness tests)


def test_e2e_infer_takes_the_vocoder_f0_from_the_model(workdir, sd_spec):
    """DiffSingerE2EInfer with the MIDI model, use_pitch_embed, use_nsf and pe_enable off: the NSF vocoder's f0 is the model's f0_denorm
    (a-*.py:629-632), compared as tests/test_gpu_infer.py compares (the oracle pipeline with the same draws, fed the device's f0)."""
    import json
    import os
    from collections import OrderedDict
    import yaml
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    from oracle import diffusion as odf, melgen as omg, nsf as onsf
    from tests.util import ROOT, maxabs
    spec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'fs2_pitch_spec.json')))['bisinger']
    sp = OrderedDict((k, tuple(s)) for k, s in spec['GaussianDiffusion'])
    full = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(sp, 0, synth.DIFFNET_GAIN).items()}
    R.make_pitch_visible(full)
    full.update(odf.make_schedule(100, 'linear', 0.06))
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'schedules.npz'))
    full['spec_min'], full['spec_max'] = torch.from_numpy(g['spec_min']), torch.from_numpy(g['spec_max'])
    for k in sp:
        if k.endswith('_float_tensor'):
            full[k] = torch.zeros(1)
    torch.save({'state_dict': {'model.' + k: v for k, v in full.items()}, 'global_step': 2000}, 'checkpoints/exp_diff_e2e/model_ckpt_steps_2000.ckpt')
    os.makedirs('checkpoints/nsf')
    nspec = OrderedDict((k, tuple(s)) for k, s in sd_spec['HifiGanGenerator_nsf_weight_norm'])
    nsd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(nspec, seed=13).items()}
    torch.save({'state_dict': {'model_gen': nsd}}, 'checkpoints/nsf/model_ckpt_steps_7.ckpt')
    hcfg = yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml'))
    hcfg['use_pitch_embed'] = True
    yaml.safe_dump(hcfg, open('checkpoints/nsf/config.yaml', 'w'))
    cfg = yaml.safe_load(open('exp.yaml'))
    cfg.update(vocoder_ckpt='checkpoints/nsf', pe_enable=False, use_nsf=True, use_pitch_embed=True, pitch_type='frame', use_uv=True,
               pitch_norm='log', pitch_ar=False, predictor_layers=5, predictor_kernel=5)
    yaml.safe_dump(cfg, open('exp3.yaml', 'w'))
    try:
        set_hparams('exp3.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=99')
        infer = DiffSingerE2EInfer(hparams)
        assert infer.vocoder.use_nsf and not hasattr(infer, 'pe') and infer.model.fs2.use_pitch_embed
        inp = _item(8, 5)
        wav = infer.infer_once(inp)
        assert wav.ndim == 1 and np.isfinite(wav).all() and np.array_equal(wav, infer.infer_once(inp))
        item = infer.preprocess_input(inp, 'phoneme')
        sample = infer.input_to_batch(item)
        out = infer._generate(sample, None)
        got_f0 = out['f0_denorm'].cpu()
        assert float((got_f0 > 0).float().mean()) > 0.1, 'the model voiced nothing: the NSF source would be noise only'
        sd = {k: v.detach().cpu() for k, v in infer.model.state_dict().items()}
        oin = {'txt_tokens': sample['txt_tokens'].cpu(), 'spk_embed': sample['spk_ids'].cpu(), 'pitch_midi': sample['pitch_midi'].cpu(),
               'midi_dur': sample['midi_dur'].cpu(), 'is_slur': sample['is_slur'].cpu(), 'lang': sample['lang'].cpu(),
               'speechsing': sample['speechsing'].cpu()}
        hp = dict(use_midi=True, use_spk_id=True, use_pitch_embed=True, use_uv=True, predictor_layers=5, predictor_kernel=5)
        # the device's own prediction as f0 / uv: one flipped bin must not enter the comparison of the waveform
        f = R.forward(sd, oin, hp, f0=out['pitch_pred'][..., 0].cpu(), uv=(out['pitch_pred'][..., 1] > 0).float().cpu())
        assert torch.equal(f['mel2ph'], out['mel2ph'].cpu())
        B, T = f['mel2ph'].shape
        n = B * 80 * T
        noise = np.stack([synth.philox_normal(99, 0, n)] + [synth.philox_normal(99, i + 1, n) for i in reversed(range(100))])
        r = omg.mel_gen(sd, oin, torch.from_numpy(noise.reshape(101, B, 80, T)), fs2_out=f)
        ri = torch.from_numpy(np.random.RandomState(99).uniform(size=(B, 9)).astype(np.float32))
        nz = torch.from_numpy(synth.philox_normal(99, 0x4E5346, B * T * 256 * 9).reshape(B, T * 256, 9))
        want = onsf.nsf_hifigan_forward(nsd, r['mel_out'].transpose(1, 2), got_f0, ri, nz, hcfg)
        assert maxabs(wav, want.reshape(-1)) <= 5e-3
        wb = infer.forward_batch([item], seed=99)
        assert len(wb) == 1 and wb[0].shape == wav.shape and maxabs(wb[0], wav) <= 1e-6
    finally:
        from tests.util import use_config
        use_config()
