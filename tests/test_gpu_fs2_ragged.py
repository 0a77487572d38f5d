"""GPU: ragged batches through the FastSpeech2 front (ABI v20: bsg_fs2midi_encode_ragged, bsg_fs2_encode_plain_ragged,
bsg_fs2_decode_ragged; FastSpeech2MIDI / FastSpeech2.forward(ragged=True), GaussianDiffusion.forward(ragged_front=True),
forward_batch(ragged_front=True)) against the float64 "alone" oracle of tests/fs2_ragged_cases.py: every row is what the front returns
for that utterance at B = 1 on its own tokens and frames.

Bounds: fs2_ragged_cases.BOUND, one per output (4 x the float32 alone oracle's own deviation from float64, measured on the CPU and held by
tests/test_fs2_ragged_cpu.py), x max(1, max |want|); f0_denorm relative to max(1, f0).  Bins are exact away from near ties
(fs2_pitch_ref.near_ties), durations away from undecided tokens (dur_cases.undecided); ties stay under 2 % of a case's real positions.
With predicted f0 everything downstream of pitch_pred is held to the oracle FED the GPU's own pitch_pred, as tests/test_gpu_fs2_pitch.py
does; with predicted durations everything downstream of mel2ph to the oracle fed the GPU's own mel2ph.
"""
import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import dur_cases as DC
from tests import fs2_pitch_ref as R
from tests import fs2_ragged_cases as RC
from tests.test_gpu_infer import _item, workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)
from tests.test_gpu_pe_ragged import nsf_workdir  # noqa: F401  (the pe_enable + use_nsf set-up)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
F64 = torch.float64
_GPU = {}


def model(front, depth, fresh=False):
    key = (front, depth)
    if fresh or key not in _GPU:
        if fresh:
            m, hp = R.build(front, depth or 2, True, None, pitch=depth is not None)
            return m.cuda(), hp, RC.model(front, depth)[2]
        m, hp, sd = RC.model(front, depth)
        _GPU[key] = (m.cuda(), hp, sd)
    return _GPU[key]


def dev(inp):
    return {k: torch.from_numpy(v).cuda() for k, v in inp.items()}


def call(m, hp, c, d, ragged=True, mel2ph=True, **kw):
    """The front's forward on the case's batch -> its dict plus enc_out (the token-level front once more: forward does not return it)."""
    mk = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')} if c.front == 'midi' else {}
    f0, uv = RC.supplied(c, d)
    spk = d['spk_embed'] if hp['use_spk_id'] else None
    got = m(d['txt_tokens'], d['mel2ph'] if mel2ph else None, spk, f0=f0 if mel2ph else None, uv=uv if mel2ph else None, infer=True,
            **({'ragged': True} if ragged else {}), **mk, **kw)
    path, rows = m.last_path().split(), m.last_rows()
    got = dict(got)
    got['enc_out'] = m.encode(d['txt_tokens'], spk, n_tok=list(c.n_tok) if ragged else None, **mk)['enc_out']
    return got, path, rows


def rows32(n, T):
    return sum(min(T, (v + 31) // 32 * 32) for v in n)


def show(what, fig):
    print(f'  {what}: ' + '  '.join(f'{k} {v:.2e} (allowed {RC.BOUND[k]:.2e})' for k, v in fig.items()))


def check_zero_beyond(c, got, n_frames=None):
    n_frames = c.n_frames if n_frames is None else n_frames
    for b in range(c.B):
        assert not got['enc_out'][b, c.n_tok[b]:].any()
        n = n_frames[b]
        for k in ('decoder_inp', 'mel_out', 'pitch_pred', 'f0_denorm', 'mel2ph'):
            if k in got:
                assert not got[k][b, n:].any(), (k, b)
        if 'pitch_bin' in got:
            assert bool((got['pitch_bin'][b, n:] == 1).all()), b


def check_frames(c, hp, sd, t, got, real):
    """The frame-level outputs of a ragged call against alone() (two stages with predicted f0); prints every figure before it asserts."""
    a64 = RC.alone(sd, hp, c, t, F64)
    fig = RC.figures(got, a64)
    if not c.depth:
        show('against float64', fig)
        assert all(fig[k] <= RC.BOUND[k] for k in fig), fig
        return
    # stage 1: pitch_pred and, away from near ties, f0_denorm and the bins
    tie, uv_tie = R.near_ties(a64, uv_tol=RC.BOUND['pitch_pred'] * max(1.0, float(a64['pitch_pred'].abs().max())))
    tie = tie if c.mode == 'pred' else torch.zeros_like(real)
    uv_tie = uv_tie if c.mode != 'f0uv' else torch.zeros_like(real)
    loose = (tie | uv_tie) & real
    f0g, f0w = got['f0_denorm'].cpu().double(), a64['f0_denorm'].double()
    fr = ((f0g - f0w).abs() / f0w.clamp(min=1))[~loose]
    print(f'  pitch_pred {fig["pitch_pred"]:.2e} (allowed {RC.BOUND["pitch_pred"]:.2e})  f0_denorm {float(fr.max()):.2e} (allowed '
          f'{RC.BOUND["f0_denorm"]:.2e})  near ties {int(loose.sum())} of {int(real.sum())}')
    assert fig['pitch_pred'] <= RC.BOUND['pitch_pred']
    assert float(loose.sum()) <= RC.TIE_CAP * float(real.sum())
    assert float(fr.max()) <= RC.BOUND['f0_denorm']
    bg = got['pitch_bin'].cpu()
    assert torch.equal(bg[~loose], a64['pitch_bin'][~loose]), 'bins differ away from a near tie'
    # stage 2: downstream of the GPU's own pitch_pred (supplied f0: of the GPU's own uv decision)
    pp = got['pitch_pred'].cpu()
    f0 = pp[..., 0] if c.mode == 'pred' else t['f0']
    uv = (pp[..., 1] > 0).float() if c.mode != 'f0uv' else t['uv']
    fed = RC.alone(sd, hp, c, t, F64, f0=f0, uv=uv)
    tie2 = (R.near_ties(fed)[0] & real) if c.mode == 'pred' else torch.zeros_like(real)
    assert float(tie2.sum()) <= RC.TIE_CAP * float(real.sum())
    assert torch.equal(bg[~tie2], fed['pitch_bin'][~tie2]) and bool(((bg - fed['pitch_bin']).abs()[tie2] <= 1).all())
    if bool((bg != fed['pitch_bin']).any()):      # a near tie that took the other neighbour: the oracle follows it
        E = sd['fs2.pitch_embed.weight'].double()
        fed['decoder_inp'] = fed['decoder_inp'] + (E[bg] - E[fed['pitch_bin']]) * real[..., None]
        fig2 = {k: v for k, v in RC.figures(got, fed).items() if k == 'decoder_inp'}
    else:
        fig2 = {k: v for k, v in RC.figures(got, fed).items() if k in ('decoder_inp', 'mel_out')}
    show('fed the GPU\'s own pitch', fig2)
    assert all(fig2[k] <= RC.BOUND[k] for k in fig2), fig2


# ------------------------------------------------------------------------------------------------------------------
# 1. every row against the utterance alone, at the shape edges
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', RC.GPU_CASES, ids=lambda c: c.name)
def test_rows_equal_the_utterance_alone(c):
    m, hp, sd = model(c.front, c.depth)
    inp = RC.inputs(c)
    t, d = RC.tensors(inp), dev(inp)
    got, path, rows = call(m, hp, c, d)
    assert m.gemm_range_take() == 0
    print(f'{c.name}: {" ".join(path)}  rows {rows}')
    assert 'tok:ragged' in path and 'dec.ragged' in path and ('esm:alone' in path) == (c.front == 'midi'), path
    assert not any(tok in path for tok in ('esm:wave', 'esm:thread', 'tok:front')), path
    if c is RC.LONG:      # the pre-split GEMMs, the QKV product's own planes and the planes attention with split keys
        assert 'dec.qkv:fused' in path and 'dec.attn:planes/ks4' in path and 'dec.gemm:h2w/64/ring8' in path, path
    # padding skipped: rows in 32-row granules (the decode's stack is the last one; the encode's rows are read after the second encode)
    assert rows[1] == rows32(c.n_frames, c.T) < c.B * c.T, rows
    assert m.last_rows() == (rows32(c.n_tok, c.Tt),) * 2
    real = t['mel2ph'] > 0
    fig = RC.figures({'enc_out': got['enc_out']}, RC.alone(sd, hp, c, t, F64))
    show('token front', fig)
    assert fig['enc_out'] <= RC.BOUND['enc_out']
    check_frames(c, hp, sd, t, got, real)
    check_zero_beyond(c, got)
    assert torch.equal(got['mel2ph'].cpu(), t['mel2ph'])


# ------------------------------------------------------------------------------------------------------------------
# 2. the launch_gemm forms (the handle's GEMMs on the fp32 matrix pipe: gemm_fast, flash_attn_kernel)
# ------------------------------------------------------------------------------------------------------------------
def test_launch_gemm_forms():
    c = RC.SMALL_GEMM
    m, hp, sd = model(c.front, c.depth, fresh=True)
    m.handle()
    m.set_gemm_split(False)
    inp = RC.inputs(c)
    t, d = RC.tensors(inp), dev(inp)
    got, path, rows = call(m, hp, c, d)
    print(' '.join(path))
    assert all(tok.split(':')[1].startswith('gemm_fast') for tok in path if '.gemm:' in tok), path
    assert 'enc.attn:flash/nw2' in path and 'dec.attn:flash/nw2' in path and 'enc.qkv:gemm' in path, path
    fig = RC.figures({'enc_out': got['enc_out']}, RC.alone(sd, hp, c, t, F64))
    show('token front', fig)
    assert fig['enc_out'] <= RC.BOUND['enc_out']
    check_frames(c, hp, sd, t, got, t['mel2ph'] > 0)
    check_zero_beyond(c, got)


# ------------------------------------------------------------------------------------------------------------------
# 3. predicted durations: dur exact away from undecided tokens, mel2ph exact given the durations, the rest fed the GPU's own mel2ph
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [RC.EDGE[0], RC.SMALL_GEMM], ids=lambda c: c.name)
def test_predicted_durations(c):
    m, hp, sd = model(c.front, c.depth)
    inp = RC.inputs(c)
    t, d = RC.tensors(inp), dev(inp)
    got, path, _ = call(m, hp, c, d, mel2ph=False)
    want = RC.alone(sd, hp, c, t, F64, predict=True)
    valid = (t['txt_tokens'] > 0).numpy()
    ref = dict(xs=want['dur'].numpy(), valid=valid, dur=want['dur_choice'].numpy())
    xs = got['dur'][..., 0].cpu().numpy()
    tol = RC.BOUND['dur'] * max(1.0, float(np.abs(ref['xs']).max()))
    print(f'  dur_xs {DC.check_xs(xs, ref, tol, c.name):.2e} (allowed {tol:.2e})')
    gd = got['dur_choice'].cpu().numpy()
    loose = DC.undecided(ref['xs'], valid, RC.BOUND['dur'])      # the tie census of tests/dur_cases.py
    print(f'  undecided tokens {int(loose.sum())} of {int(valid.sum())}')
    assert int(loose.sum()) <= RC.TIE_CAP * int(valid.sum())
    assert np.array_equal(gd[~loose], ref['dur'][~loose]), 'dur differs on decided tokens'
    lo, hi = DC.neighbours(ref['xs'])
    assert bool(((gd == lo) | (gd == hi))[loose].all())
    n_frames = [int(v) for v in gd.sum(-1)]
    T = max(n_frames)
    assert np.array_equal(got['mel2ph'].cpu().numpy(), DC.regulate_ref(gd, None, T))
    # downstream of the GPU's own mel2ph
    c2 = RC.Case(c.front, c.depth, c.B, c.Tt, T, c.n_tok, n_frames, 'pred')
    t2 = dict(t, mel2ph=got['mel2ph'].cpu(), f0=torch.zeros(c.B, T), uv=torch.zeros(c.B, T))
    check_frames(c2, hp, sd, t2, got, t2['mel2ph'] > 0)
    check_zero_beyond(c2, got, n_frames)
    assert not got['dur'][..., 0].cpu().numpy()[~valid].any() and not gd[~valid].any()


# ------------------------------------------------------------------------------------------------------------------
# 4. nothing beyond a row's end, and no other row, reaches a row
# ------------------------------------------------------------------------------------------------------------------
KEYS = ('enc_out', 'decoder_inp', 'mel_out', 'pitch_pred', 'f0_denorm', 'pitch_bin')


def same(a, b, rows=None):
    return all(torch.equal(a[k] if rows is None else a[k][rows], b[k] if rows is None else b[k][rows]) for k in KEYS if k in a)


@pytest.mark.parametrize('c', [RC.EDGE[0], RC.EDGE[1], RC.EDGE[2]], ids=lambda c: c.name)
def test_padding_and_other_rows_never_reach_a_row(c):
    m, hp, sd = model(c.front, c.depth)
    inp = RC.inputs(c)
    clean, _, _ = call(m, hp, c, dev(inp))
    # NaN / ids far outside their tables in every input beyond a row's end, NaN bytes over the workspace before the call
    m.poison_workspace()
    dirty, _, _ = call(m, hp, c, dev(RC.garbage(c, inp)))
    assert m.gemm_range_take() == 0
    assert same(clean, dirty), [k for k in KEYS if k in clean and not torch.equal(clean[k], dirty[k])]
    # the same with txt_tokens and mel2ph replaced beyond the ends too, through the calls that are given the lengths
    g = dev(RC.garbage(c, inp, ends=True))
    mk = {k: g[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang')} if c.front == 'midi' else {}
    spk = g['spk_embed'] if hp['use_spk_id'] else None
    f0, uv = RC.supplied(c, g)
    m.poison_workspace()
    enc = m.encode(g['txt_tokens'], spk, n_tok=list(c.n_tok), **mk)['enc_out']
    low = dict(m.decode_all(enc, g['mel2ph'], spk, g['speechsing'] if c.front == 'midi' else None, f0=f0, uv=uv, n_tok=list(c.n_tok),
                            n_frames=list(c.n_frames)), enc_out=enc)
    assert same(clean, low), [k for k in KEYS if k in clean and not torch.equal(clean[k], low[k])]
    # another content in row 0 (same lengths): the other rows are bit-identical, row 0 is not
    other = RC.inputs(RC.Case(c.front, c.depth, c.B, c.Tt, c.T, c.n_tok, c.n_frames, c.mode, seed=c.seed + 1))
    mixed = {k: v.copy() for k, v in inp.items()}
    for k in RC.TOKEN_KEYS + ('f0', 'uv'):
        mixed[k][0] = other[k][0]
    moved, _, _ = call(m, hp, c, dev(mixed))
    assert same(clean, moved, slice(1, None)) and not torch.equal(clean['mel_out'][0], moved['mel_out'][0])


def test_short_call_after_long_one_equals_a_fresh_handle():
    m, hp, sd = model('midi', 2)
    call(m, hp, RC.MANY, dev(RC.inputs(RC.MANY)))
    m.poison_workspace()
    a, _, _ = call(m, hp, RC.SMALL_GEMM, dev(RC.inputs(RC.SMALL_GEMM)))
    fresh, fhp, _ = model('midi', 2, fresh=True)
    b, _, _ = call(fresh, fhp, RC.SMALL_GEMM, dev(RC.inputs(RC.SMALL_GEMM)))
    assert same(a, b)


CAPTURE = [RC.Case('plain', 2, 3, 33, 65, (33, 2, 9), (65, 0, 31), 'f0uv'),      # a row without frames
           RC.Case('midi', 2, 3, 33, 65, (33, 2, 9), (65, 4, 31), 'pred')]          # the ESM table and the ragged embedding launch


@pytest.mark.parametrize('c', CAPTURE, ids=lambda c: c.name)
def test_zero_frame_row_and_captured_replay(c):
    """A row whose frames are none (what predicted durations that sum to 0 give) is zeros and disturbs nobody; the second run of a shape,
    captured and replayed, is bit-identical to the eager one — on the plain front and on the MIDI front, whose ragged encode adds the ESM
    table's launches and embed_ragged_kernel."""
    m, hp, sd = model(c.front, c.depth)
    inp = RC.inputs(c)
    t, d = RC.tensors(inp), dev(inp)
    eager, _, _ = call(m, hp, c, d)
    check_frames(c, hp, sd, t, eager, t['mel2ph'] > 0)
    check_zero_beyond(c, eager)
    nt, nf = list(c.n_tok), list(c.n_frames)
    mk = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang')} if c.front == 'midi' else {}
    spk = d['spk_embed'] if hp['use_spk_id'] else None
    f0, uv = RC.supplied(c, d)

    def both():
        enc = m.encode(d['txt_tokens'], spk, n_tok=nt, **mk)['enc_out']
        return dict(m.decode_all(enc, d['mel2ph'], spk, d['speechsing'] if c.front == 'midi' else None, f0=f0, uv=uv, n_tok=nt, n_frames=nf),
                    enc_out=enc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        both()       # warm-up on the side stream (workspaces are sized)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = both()
    for v in cap.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same(eager, cap), [k for k in KEYS if k in eager and not torch.equal(eager[k], cap[k])]
    if c.front == 'midi':
        assert 'esm:alone' in m.last_path() and 'tok:ragged' in m.last_path()


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals: BSG_EINVAL with a message before any device call; ValueError for a row that is no prefix
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    c = RC.EDGE[1]
    m, hp, sd = model(c.front, c.depth)
    d = dev(RC.inputs(c))
    good, _, _ = call(m, hp, c, d)
    lib = _lib.load()
    for nt, msg in (([33, 0, 9], r'n_tok_host\[1\]=0 outside 1\.\.33'), ([33, 2, 34], r'n_tok_host\[2\]=34 outside 1\.\.33')):
        with pytest.raises(_lib.BsgError, match=msg):
            m.encode(d['txt_tokens'], None, n_tok=nt)
    enc = good['enc_out']
    for nf, msg in (([65, -1, 31], r'n_frames_host\[1\]=-1 outside 0\.\.65'), ([66, 4, 31], r'n_frames_host\[0\]=66 outside 0\.\.65')):
        with pytest.raises(_lib.BsgError, match=msg):
            m.decode_all(enc, d['mel2ph'], None, None, f0=d['f0'], uv=d['uv'], n_tok=list(c.n_tok), n_frames=nf)
    out = torch.full((c.B, c.Tt, 256), 7.0, device='cuda')
    rc_ = lib.bsg_fs2_encode_plain_ragged(m.handle(), _lib.ptr(d['txt_tokens']), None, None, c.B, c.Tt, _lib.ptr(out), None, None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc_ == -22 and 'n_tok_host is null' in lib.bsg_last_error().decode() and bool((out == 7.0).all())
    with pytest.raises(_lib.BsgError, match='the handle has the plain front'):
        _lib.check(lib.bsg_fs2midi_encode_ragged(m.handle(), *([_lib.ptr(d['txt_tokens'])] * 6), (_lib.c_int32 * c.B)(*c.n_tok), c.B, c.Tt,
                                                 _lib.ptr(out), None, None, _lib.stream_ptr()), 'bsg_fs2midi_encode_ragged')
    hole = d['txt_tokens'].clone()
    hole[0, 3] = 0
    with pytest.raises(ValueError, match='row 0 of txt_tokens'):
        m(hole, d['mel2ph'], None, infer=True, ragged=True)
    m2p = d['mel2ph'].clone()
    m2p[2, 0] = 0
    with pytest.raises(ValueError, match='row 2 of mel2ph'):
        m(d['txt_tokens'], m2p, None, infer=True, ragged=True)
    with pytest.raises(NotImplementedError, match='rows'):
        m(d['txt_tokens'], d['mel2ph'], None, infer=True, ragged=True, rows=slice(0, 1))
    again, _, _ = call(m, hp, c, d)      # the handle is as usable as before
    assert same(good, again)


# ------------------------------------------------------------------------------------------------------------------
# 6. GaussianDiffusion.forward(ragged_front=True) and forward_batch(ragged_front=True)
# ------------------------------------------------------------------------------------------------------------------
def _diffusion(adaptor):
    """GaussianDiffusion (4 DDPM steps) around the MIDI front, formula weights, durations of a few frames per token; adaptor: the 2-layer
    frame-level pitch adaptor with its pitch made visible (fs2_pitch_ref.make_pitch_visible)."""
    from bisinger_amd.diffnet import DIFF_DECODERS
    from bisinger_amd.diffusion import GaussianDiffusion
    from bisinger_amd.hparams import hparams
    from tests import cfg_fixtures
    from tests.util import load_formula_weights, use_config
    use_config('timesteps=4,K_step=4,max_beta=0.06,pndm_speedup=0')
    try:
        if adaptor:
            hparams.update(use_pitch_embed=True, use_uv=True, pitch_type='frame', predictor_layers=2, predictor_kernel=5)
        m = GaussianDiffusion(R.PhoneEncoder(), 80, DIFF_DECODERS[hparams['diff_decoder_type']](hparams), timesteps=4, K_step=4,
                              spec_min=hparams['spec_min'], spec_max=hparams['spec_max'])
        load_formula_weights(m, 0, cfg_fixtures.CFG0['gain'])
        if adaptor:
            R.make_pitch_visible(dict(m.state_dict()))      # (in place on the module's own tensors; raises the duration bias too)
        else:
            m.fs2.dur_predictor.linear.bias.data.add_(1.8)      # (tests/dur_cases.py RAISE: the formula weights round half the durations to 0)
        return m.cuda().eval()
    finally:
        use_config()


@pytest.mark.parametrize('adaptor', [False, True], ids=['no-adaptor', 'adaptor-L2'])
def test_gaussian_diffusion_ragged_front_rows_equal_its_own_lone_calls(adaptor):
    """Row by row against the same model's own B = 1 padded calls, with given and with predicted mel2ph: decoder_inp, fs2_mel and dur_choice,
    and with the adaptor pitch_pred, f0_denorm (relative to max(1, f0)) and pitch_bin — each within fs2_ragged_cases.BOUND, the bound of the
    float64 comparison, although both sides are fp32 here.  Frames whose uv logit or bin lies within the bound of a rounding edge (a near
    tie of the lone call; at most 2 % of a row) may fall either way and are left out of f0_denorm / pitch_bin; a row in which one did is
    held on decoder_inp away from that frame only."""
    m = _diffusion(adaptor)
    c = RC.Case('midi', 2 if adaptor else None, 3, 12, 64, (12, 5, 9), (64, 31, 33), 'pred')
    d = dev(RC.inputs(c))
    names = ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')
    kw = lambda b, nt: {k: (d[k][b:b + 1, :nt] if d[k].dim() == 2 else d[k][b:b + 1]) for k in names}
    full = {k: d[k] for k in names}
    for given in (True, False):
        got = m(d['txt_tokens'], d['mel2ph'] if given else None, d['spk_embed'], infer=True, ragged_front=True, seed=3, **full)
        assert torch.isfinite(got['mel_out']).all()
        for b in range(c.B):
            nt = c.n_tok[b]
            n = c.n_frames[b] if given else int((got['mel2ph'][b] > 0).sum())
            lone = m(d['txt_tokens'][b:b + 1, :nt], d['mel2ph'][b:b + 1, :n] if given else None, d['spk_embed'][b:b + 1], infer=True, seed=3, **kw(b, nt))
            if not given:
                assert torch.equal(got['dur_choice'][b, :nt], lone['dur_choice'][0]) and lone['mel2ph'].shape[1] == n and n > 0
                assert not got['dur_choice'][b, nt:].any()
            clean = torch.ones(n, dtype=torch.bool, device='cuda')
            if adaptor:
                pw = lone['pitch_pred'][0].double()
                scale = max(1.0, float(pw.abs().max()))
                err = float((got['pitch_pred'][b, :n].double() - pw).abs().max()) / scale
                print(f'  given={given} row {b} pitch_pred: {err:.2e} (allowed {RC.BOUND["pitch_pred"]:.2e})')
                assert err <= RC.BOUND['pitch_pred']
                f0w = lone['f0_denorm'][0].double()
                x = R.f0_to_mel_bins(f0w)[0] + 0.5
                tie = ((x - torch.round(x)).abs() < RC.BOUND["pitch_pred"] * 125 + 1e-3) | (pw[:, 1].abs() < RC.BOUND['pitch_pred'] * scale)
                assert float(tie.sum()) <= RC.TIE_CAP * n
                fr = ((got['f0_denorm'][b, :n].double() - f0w).abs() / f0w.clamp(min=1))[~tie]
                print(f'  given={given} row {b} f0_denorm: {float(fr.max()):.2e} (allowed {RC.BOUND["f0_denorm"]:.2e})  near ties {int(tie.sum())} of {n}')
                assert float(fr.max()) <= RC.BOUND['f0_denorm']
                assert torch.equal(got['pitch_bin'][b, :n][~tie], lone['pitch_bin'][0][~tie])
                clean = got['pitch_bin'][b, :n] == lone['pitch_bin'][0]
                assert not got['pitch_pred'][b, n:].any() and not got['f0_denorm'][b, n:].any() and bool((got['pitch_bin'][b, n:] == 1).all())
            for k in ('decoder_inp', 'fs2_mel'):
                if k == 'fs2_mel' and not bool(clean.all()):
                    print(f'  given={given} row {b}: a near tie took the other bin; fs2_mel (downstream of it through the attention) is not compared')
                    continue
                bound = RC.BOUND['mel_out' if k == 'fs2_mel' else k]
                err = float((got[k][b, :n] - lone[k][0])[clean].abs().max()) / max(1.0, float(lone[k].abs().max()))
                print(f'  given={given} row {b} {k}: {err:.2e} (allowed {bound:.2e})')
                assert err <= bound and not got[k][b, n:].any()
    with pytest.raises(NotImplementedError, match='ragged_front'):
        m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], infer=True, ragged_front=True, rows=slice(0, 1), **full)


def test_forward_batch_every_ragged_switch(nsf_workdir):  # noqa: F811
    # (shapes and path tokens only; the values of this call, stage by stage against float64 on the utterance alone: tests/test_gpu_e2e_ragged.py)
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp2.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=99')
    infer = DiffSingerE2EInfer(hparams)
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3))]
    wavs = infer.forward_batch(items, seed=77, ragged_front=True, ragged=True, ragged_pitch=True, ragged_vocoder=True)
    path = infer.model.fs2.last_path().split()
    assert 'esm:alone' in path and 'tok:ragged' in path and 'dec.ragged' in path, path
    hop = int(np.prod(infer.vocoder.h['upsample_rates']))
    frames = infer.last_batch_stats['frames']
    for w, n in zip(wavs, frames):
        assert w.shape == (n * hop,) and np.isfinite(w).all() and n > 0
    padded = infer.forward_batch(items, seed=77, ragged=True, ragged_pitch=True, ragged_vocoder=True)      # the default front: unchanged tokens
    assert 'esm:alone' not in infer.model.fs2.last_path() and len(padded) == len(wavs)
