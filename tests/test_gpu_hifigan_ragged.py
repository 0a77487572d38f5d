"""GPU: ragged batches through the HiFi-GAN generator (bsg_hifigan_forward_ragged / _nsf_ragged, HifiGanGenerator.forward(lengths=)).

A ragged forward runs the plan, the grids and the launches of the padded call at (B, T); every launch bounds row b by lengths[b] x (the
upsample rates so far) instead of by the stage length.  What is checked:

  1. every row against the float64 oracle run on THAT ROW ALONE (mel[b, :, :n_b]; never the padded oracle), over the row's whole n_b x 256
     samples and, separately, over its first and last 256, where the new bound lives.  Bar: that of tests/test_gpu_hifigan_shapes.py for
     these weights and inputs, 5.4e-6 x max(1, max |want|); the fp32 oracle's own deviation on the same rows is printed as the yardstick.
     The inputs beyond each row's end (mel; NSF: f0 and noise too) are NaN, the workspace is filled with NaN bytes before the forward
     (bsg_hifigan_debug_poison_workspace): the output must be finite, and exactly 0 beyond n_b x 256.  Shapes from the dispatch map of that
     file so that every default form runs with a row end inside a tile; the fallback switch sets run (3, 683) in child processes;
  2. all lengths = T is the padded call bit for bit, last_path differing by the leading token `ragged` only;
  3. a row's samples do not change when the other rows do;
  4. a captured ragged forward replays bit-identically; a short ragged call after a long padded one on a poisoned workspace equals a
     fresh handle;
  5. refusals (also tests/test_hifigan_ragged_cpu.py);
  6. forward_batch(ragged_vocoder=True) end to end: each waveform against the vocoder run on that row's own mel alone.

Every case asserts that no range event fired.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from oracle import hifigan as ohg, nsf as onsf
from tests.test_gpu_f2_fullsize import notes_f0, nsf  # noqa: F401  (nsf: the module-scoped NSF generator fixture of that file)
from tests.test_gpu_hifigan_shapes import BAR, EDGE, _maxabs, _mel, _run_guarded, plain, rb2  # noqa: F401  (plain, rb2: generator fixtures)
from tests.test_gpu_infer import _item, workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

F64, F32 = torch.float64, torch.float32
HOP, NH = 256, 9

PLAIN_CASES = [
    (4, 5, [5, 1, 3, 2]),                                        # rows shorter than every halo: polyphase, NC4, NB1
    (3, 683, [683, 7, 342]),                                     # upk, up2 with a partial tile, NC8, NB2
    (8, 1001, [1001, 1000, 999, 513, 512, 511, 64, 1]),          # up2, NB2: ends on, before and after the 1024-sample and 256-position seams
    (64, 33, [1 + (b % 33) for b in range(64)]),
]
LENS_683 = [683, 7, 342]

_REF = {}      # (kind, B, T) -> per-row float64 / fp32 references on the row alone, computed once


def _nan_tail(a, lens, axis_scale=1):
    """a [B, ..., T x axis_scale] (time last) or [B, L, NH] handled by the caller: NaN at and beyond each row's end."""
    a = a.copy()
    for b, n in enumerate(lens):
        a[b, ..., n * axis_scale:] = np.nan
    return a


def _plain_rows(sd, cfg, B, T, lens, kind='plain', mel=None):
    key = (kind, B, T, tuple(lens))
    if key not in _REF:
        mel = _mel(B, T) if mel is None else mel
        want, dev32 = [], 0.0
        for b, n in enumerate(lens):
            m = torch.from_numpy(mel[b:b + 1, :, :n].copy())
            w = ohg.hifigan_forward(sd, m, cfg, dtype=F64).numpy()[0, 0]
            dev32 = max(dev32, _maxabs(ohg.hifigan_forward(sd, m, cfg, dtype=F32).double().numpy()[0, 0], w))
            want.append(w)
        _REF[key] = dict(mel=mel, want=want, dev32=dev32)
    return _REF[key]


def _check_rows(tag, got, want, lens, T, dev32=None):
    """got [B, 1, T HOP] float64; want: list of the rows' own references."""
    assert got.shape == (len(lens), 1, T * HOP), (tag, got.shape)
    assert np.isfinite(got).all(), tag
    worst = worst_edge = 0.0
    for b, n in enumerate(lens):
        row, w = got[b, 0], want[b]
        assert w.shape == (n * HOP,)
        assert not row[n * HOP:].any(), (tag, b, 'samples beyond the row end are not 0')
        bar = BAR * max(1.0, float(np.abs(w).max()))
        dev = _maxabs(row[:n * HOP], w)
        edge = max(_maxabs(row[:EDGE], w[:EDGE]), _maxabs(row[max(0, n * HOP - EDGE):n * HOP], w[-EDGE:]))
        worst, worst_edge = max(worst, dev), max(worst_edge, edge)
        assert dev <= bar, (tag, b, n, dev, bar)
        assert edge <= bar, (tag, b, n, edge, bar)
    print(f'\nhifigan ragged {tag}: hip {worst:.2e} edge {worst_edge:.2e}' + ('' if dev32 is None else f' | fp32 oracle on the same rows {dev32:.2e}'))


def _ragged_tokens(path):
    tok = path.split()
    assert tok[0] == 'ragged', path
    return tok[1:]


# ------------------------------------------------------------------------------------------------------------------
# 1. every row alone, against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,lens', PLAIN_CASES, ids=[f'{c[0]}x{c[1]}' for c in PLAIN_CASES])
def test_plain_rows_alone_vs_fp64(B, T, lens, plain):  # noqa: F811
    gen, sd, cfg = plain
    ref = _plain_rows(sd, cfg, B, T, lens)
    _, padded_path = _run_guarded(gen, torch.from_numpy(ref['mel']).cuda())
    gen.poison_workspace()
    got, path = _run_guarded(gen, torch.from_numpy(_nan_tail(ref['mel'], lens)).cuda(), lengths=lens)
    assert _ragged_tokens(path) == padded_path.split(), (path, padded_path)
    _check_rows(f'plain {B}x{T}', got, ref['want'], lens, T, ref['dev32'])


def _f0(rs, B, T):
    if T >= 50:
        return np.stack([notes_f0(rs, T) for _ in range(B)])
    f0 = np.full((B, T), 220.0, np.float32)
    if B > 1:
        f0[1, 0] = 0
    return f0


@pytest.mark.parametrize('B,T,lens', [(2, 5, [5, 2]), (2, 601, [601, 300])], ids=['2x5', '2x601'])
def test_nsf_rows_alone_vs_fp64(B, T, lens, nsf):  # noqa: F811
    gen, sd, cfg = nsf
    rs = np.random.RandomState(500 * B + T)
    mel = (rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
    f0 = _f0(rs, B, T)
    rand_ini = rs.uniform(0, 1, size=(B, NH)).astype(np.float32)
    noise = rs.standard_normal((B, T * HOP, NH)).astype(np.float32)
    want, dev32 = [], 0.0
    for b, n in enumerate(lens):
        args = (sd, torch.from_numpy(mel[b:b + 1, :, :n].copy()), torch.from_numpy(f0[b:b + 1, :n].copy()), torch.from_numpy(rand_ini[b:b + 1]),
                torch.from_numpy(noise[b:b + 1, :n * HOP].copy()), cfg)
        w = onsf.nsf_hifigan_forward(*args, dtype=F64).numpy()[0, 0]
        dev32 = max(dev32, _maxabs(onsf.nsf_hifigan_forward(*args, dtype=F32).double().numpy()[0, 0], w))
        want.append(w)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    _, padded_path = _run_guarded(gen, dev(mel), dev(f0), rand_ini=torch.from_numpy(rand_ini), noise=torch.from_numpy(noise))
    noise_nan = noise.copy()
    for b, n in enumerate(lens):
        noise_nan[b, n * HOP:] = np.nan
    gen.poison_workspace()
    got, path = _run_guarded(gen, dev(_nan_tail(mel, lens)), dev(_nan_tail(f0, lens)), rand_ini=torch.from_numpy(rand_ini), noise=torch.from_numpy(noise_nan),
                             lengths=lens)
    assert _ragged_tokens(path) == padded_path.split(), (path, padded_path)
    _check_rows(f'nsf {B}x{T}', got, want, lens, T, dev32)


def test_resblock2_rows_alone_vs_fp64(rb2):  # noqa: F811
    gen, sd, cfg = rb2
    B, T, lens = 2, 5, [5, 3]
    mel = (np.random.RandomState(700 * B + T).standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
    ref = _plain_rows(sd, cfg, B, T, lens, kind='rb2', mel=mel)
    _, padded_path = _run_guarded(gen, torch.from_numpy(mel).cuda())
    gen.poison_workspace()
    got, path = _run_guarded(gen, torch.from_numpy(_nan_tail(mel, lens)).cuda(), lengths=lens)
    assert _ragged_tokens(path) == padded_path.split(), (path, padded_path)
    _check_rows(f'rb2 {B}x{T}', got, ref['want'], lens, T, ref['dev32'])


CHILD = r'''
import sys, json, torch, numpy as np
sys.path.insert(0, %r)
import bench
from bisinger_amd import _lib
torch.set_grad_enabled(False)
voc, cfg = bench.build_vocoder(torch.device('cuda', 0))      # formula weights of seed 7 = the hifigan_sd fixture, weight norm folded
f, lens = sys.argv[1], json.loads(sys.argv[2])
mel = np.load(f + '.mel.npy')
y = voc(torch.from_numpy(np.nan_to_num(mel, nan=-3.0)).cuda())
padded = voc.last_path()
voc.poison_workspace()
y = voc(torch.from_numpy(mel).cuda(), lengths=lens)
np.save(f + '.out.npy', y.cpu().numpy())
print(json.dumps({'path': voc.last_path(), 'padded': padded, 'retries': _lib.range_retries, 'events': voc.gemm_range_peek()}))
''' % ROOT

FALLBACKS = {
    'fp32_mfma': {'BSG_HG_SPLIT': '0'},
    'valu': {'BSG_HG_MFMA': '0'},
    'vector_convs': {'BSG_HG_H2W': '0', 'BSG_NO_CONV_POST': '1', 'BSG_NO_UP2': '1'},
    'unfused': {'BSG_HG_FUSED': '0', 'BSG_HG_CHAIN': '0'},
}


@pytest.mark.parametrize('name', list(FALLBACKS))
def test_fallback_forms_rows_alone_vs_fp64(name, tmp_path, plain):  # noqa: F811
    """The fallback switch sets of tests/test_gpu_hifigan_shapes.py (one child process per set: the switches are read once per process)
    at (3, 683) with row ends inside the tiles."""
    gen, sd, cfg = plain
    B, T, lens = 3, 683, LENS_683
    ref = _plain_rows(sd, cfg, B, T, lens)
    f = str(tmp_path / 'case')
    np.save(f + '.mel.npy', _nan_tail(ref['mel'], lens))
    res = subprocess.run([sys.executable, '-c', CHILD, f, json.dumps(lens)], env=dict(os.environ, **FALLBACKS[name]), capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, (name, res.stderr[-2000:])
    r = json.loads(res.stdout.strip().splitlines()[-1])
    assert r['retries'] == 0 and r['events'] == 0, (name, r)
    assert _ragged_tokens(r['path']) == r['padded'].split(), (name, r)
    _check_rows(f'{name} {B}x{T}', np.load(f + '.out.npy').astype(np.float64), ref['want'], lens, T, ref['dev32'])


# ------------------------------------------------------------------------------------------------------------------
# 2. all lengths = T is the padded call
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,T', [(2, 999), (16, 1000)])
def test_full_lengths_are_the_padded_call_plain(B, T, plain):  # noqa: F811
    gen = plain[0]
    mel = torch.from_numpy(_mel(B, T)).cuda()
    want, padded_path = _run_guarded(gen, mel)
    gen.poison_workspace()
    got, path = _run_guarded(gen, mel, lengths=[T] * B)
    assert np.array_equal(got, want), _maxabs(got, want)
    assert path == 'ragged ' + padded_path


@pytest.mark.parametrize('B,T', [(2, 999), (16, 1000)])
def test_full_lengths_are_the_padded_call_nsf(B, T, nsf):  # noqa: F811
    gen = nsf[0]
    rs = np.random.RandomState(B + T)
    mel = torch.from_numpy((rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)).cuda()
    f0 = torch.from_numpy(np.stack([notes_f0(rs, T) for _ in range(B)])).cuda()
    want, padded_path = _run_guarded(gen, mel, f0, seed=5)
    gen.poison_workspace()
    got, path = _run_guarded(gen, mel, f0, seed=5, lengths=torch.tensor([T] * B))
    assert np.array_equal(got, want), _maxabs(got, want)
    assert path == 'ragged ' + padded_path


# ------------------------------------------------------------------------------------------------------------------
# 3. rows do not see each other
# ------------------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_itself_alone(plain):  # noqa: F811
    gen = plain[0]
    B, T = 3, 683
    mel = _mel(B, T)
    a, _ = _run_guarded(gen, torch.from_numpy(mel).cuda(), lengths=[683, 7 + 300, 342])
    other = mel.copy()
    other[0], other[2] = _mel(B, T + 1)[0, :, :T] * 0.5, _mel(B, T + 2)[2, :, :T] + 1.0
    b, _ = _run_guarded(gen, torch.from_numpy(other).cuda(), lengths=[12, 7 + 300, 683])
    assert np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------------------------
# 4. capture; a short ragged call after a long padded one
# ------------------------------------------------------------------------------------------------------------------
def test_captured_ragged_forward_replays(plain):  # noqa: F811
    gen = plain[0]
    B, T, lens = 3, 683, LENS_683
    mel = torch.from_numpy(_mel(B, T)).cuda()
    eager, path = _run_guarded(gen, mel, lengths=lens)
    hd, lib = gen.handle(), _lib.load()
    arr = (__import__('ctypes').c_int32 * B)(*lens)
    y = torch.empty(B, 1, T * HOP, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.check(lib.bsg_hifigan_forward_ragged(hd, _lib.ptr(mel), arr, _lib.ptr(y), B, T, _lib.stream_ptr()), 'warm-up')
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.bsg_hifigan_forward_ragged(hd, _lib.ptr(mel), arr, _lib.ptr(y), B, T, _lib.stream_ptr()), 'capture')
    for i in range(B):
        arr[i] = 1                  # the host array is read before the call returns: the replay keeps the captured counts
    gen.poison_workspace()
    y.fill_(float('nan'))
    g.replay()
    torch.cuda.synchronize()
    assert gen.gemm_range_peek() == 0
    assert np.array_equal(y.double().cpu().numpy(), eager)
    assert gen.last_path() == path


def test_short_ragged_after_long_padded_equals_fresh_handle(plain, hifigan_sd):  # noqa: F811
    import yaml
    from bisinger_amd.hifigan import HifiGanGenerator
    gen = plain[0]
    _run_guarded(gen, torch.from_numpy(_mel(16, 1000)).cuda())
    gen.poison_workspace()
    B, T, lens = 3, 683, LENS_683
    mel = torch.from_numpy(_nan_tail(_mel(B, T), lens)).cuda()
    got, path = _run_guarded(gen, mel, lengths=lens)
    fresh = HifiGanGenerator(yaml.safe_load(open(f'{ROOT}/bisinger_amd/configs/hifigan.yaml')))
    fresh.load_state_dict(hifigan_sd, strict=True)
    fresh = fresh.cuda()
    want, fresh_path = _run_guarded(fresh, mel, lengths=lens)
    fresh.release()
    assert np.array_equal(got, want), _maxabs(got, want)
    assert path == fresh_path


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(plain, nsf):  # noqa: F811
    import ctypes
    gen = plain[0]
    B, T = 2, 5
    mel = torch.from_numpy(_mel(B, T)).cuda()
    gen(mel)
    hd, lib = gen.handle(), _lib.load()
    for lens, row in (([5, 0], 1), ([6, 5], 0), ([5, -3], 1)):
        y = torch.full((B, 1, T * HOP), 7.0, device='cuda')
        rc = lib.bsg_hifigan_forward_ragged(hd, _lib.ptr(mel), (ctypes.c_int32 * B)(*lens), _lib.ptr(y), B, T, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -22, (lens, rc)
        msg = lib.bsg_last_error().decode()
        assert f'lengths[{row}]={lens[row]}' in msg and f'1..T={T}' in msg, msg
        assert bool((y == 7.0).all()), lens
        with pytest.raises(_lib.BsgError, match=rf'lengths\[{row}\]={lens[row]} outside 1\.\.T={T}'):
            gen(mel, lengths=lens)
    with pytest.raises(_lib.BsgError, match='lengths has 3 entries for a batch of 2 rows'):
        gen(mel, lengths=[5, 5, 5])
    rc = lib.bsg_hifigan_forward_ragged(hd, _lib.ptr(mel), None, _lib.ptr(mel), B, T, _lib.stream_ptr())
    assert rc == -22 and 'lengths_host is null' in lib.bsg_last_error().decode()
    # the NSF entry point on a plain handle and the other way round
    y = torch.full((B, 1, T * HOP), 7.0, device='cuda')
    arr = (ctypes.c_int32 * B)(5, 5)
    rc = lib.bsg_hifigan_forward_ragged(nsf[0].handle(), _lib.ptr(mel), arr, _lib.ptr(y), B, T, _lib.stream_ptr())
    assert rc == -22 and 'NSF' in lib.bsg_last_error().decode()
    rc = lib.bsg_hifigan_forward_nsf_ragged(hd, _lib.ptr(mel), _lib.ptr(mel), _lib.ptr(mel), _lib.ptr(mel), arr, _lib.ptr(y), B, T, _lib.stream_ptr())
    assert rc == -22 and 'without the NSF source' in lib.bsg_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------
# 6. end to end
# ------------------------------------------------------------------------------------------------------------------
def test_forward_batch_ragged_vocoder(workdir):  # noqa: F811
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    infer = DiffSingerE2EInfer(hparams)
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3), (4, 4), (7, 5))]
    voc = infer.vocoder
    calls = []
    inner = voc.forward

    def recording(x, *a, **kw):
        calls.append((x.clone(), kw.get('lengths')))
        return inner(x, *a, **kw)
    voc.forward = recording
    before = _lib.range_retries
    wavs = infer.forward_batch(items, seed=77, max_sentences=3, ragged=True, ragged_vocoder=True)
    st = infer.last_batch_stats
    ragged_calls, calls[:] = list(calls), []
    today = infer.forward_batch(items, seed=77, max_sentences=3, ragged=True)
    explicit = infer.forward_batch(items, seed=77, max_sentences=3, ragged=True, ragged_vocoder=False)
    padded_calls = list(calls)
    voc.forward = inner
    assert len(ragged_calls) == len(st['buckets']) == 2 and len(padded_calls) == 4
    assert all(c[1] is None for c in padded_calls)
    worst = 0.0
    for bk, (mel, lens) in zip(st['buckets'], ragged_calls):
        assert list(lens) == [st['frames'][i] for i in bk]
        padded = voc(mel)[:, 0]
        for r, i in enumerate(bk):
            n = st['frames'][i]
            want = voc(mel[r:r + 1, :, :n].contiguous())[0, 0].double().cpu().numpy()      # the vocoder on that row's own mel alone (B = 1, T = n)
            assert wavs[i].shape == (n * HOP,) and np.isfinite(wavs[i]).all()
            dev = _maxabs(wavs[i], want)
            worst = max(worst, dev)
            assert dev <= 5e-5 * max(1.0, float(np.abs(want).max())), (i, n, dev)
            # the padded vocoder batch is what forward_batch gives without ragged_vocoder, bit for bit, given as a keyword or not
            assert np.array_equal(today[i], padded[r, :n * HOP].cpu().numpy())
            assert np.array_equal(explicit[i], today[i])
    print(f'\nforward_batch(ragged_vocoder=True): worst deviation from the rows alone {worst:.2e}')
    assert _lib.range_retries == before and voc.gemm_range_peek() == 0
    hparams['vocoder'] = 'pwg'
    try:
        with pytest.raises(NotImplementedError, match='pwg'):
            infer.forward_batch(items, seed=77, max_sentences=3, ragged_vocoder=True)
    finally:
        hparams['vocoder'] = 'vocoders.hifigan.HifiGAN'
