"""GPU: ragged batches through the Parallel WaveGAN generator (bsg_pwg_forward_ragged, csrc/pwg.hip) — every row as the generator applied
to that utterance alone.  The handle, the formula weights and the float64 restatement are those of tests/test_gpu_pwg.py.

The contract is bit equality with the lone call (bsg_pwg_forward at B = 1, T = n_b on the row's own edge-padded mel), so most tests here
have no tolerance at all.  The one that has (test_rows_against_float64) is independent of the padded kernel: every row of CASE1 (hop 256,
both forms) and of CASE2 (hop 300, the small generator of test_partial_tiles_with_a_hop_of_300) against tests/pwg_ref.forward in float64
on that row alone, under the rule of tests/test_gpu_pwg.py: ONE number per weight set, 4 x the largest err_fp32 (the restatement in
float32 against float64) over this file's rows of that set, computed on the CPU before the kernel runs, x max(1, max |want|) of the row;
no row excluded.  Measured (bound, then the kernel's largest error / max(1, max |want|)):
    plain, hop 256 (CASE1)   bound 3.250e-06    kernel 8.157e-07
    pitch, hop 256 (CASE1)   bound 1.291e-06    kernel 2.964e-07
    plain, hop 300 (CASE2)   bound 1.332e-06    kernel 3.903e-07
Drawn noise (z == NULL) against the host's Philox stream fed in: 5e-6 on the waveform, the figure of
test_philox_noise_equals_the_host_stream_fed_in; measured 3.278e-07 (plain), 1.937e-07 (pitch)."""
import functools
from collections import OrderedDict
from ctypes import Array, c_int32

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import pwg_ref as ref
from tests.test_gpu_pwg import FORMS, PHILOX_STREAM, Gen, expected_path, weights

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

W = 2                                              # aux_context_window
CASE1 = (5, 9, (9, 1, 2, 7, 3))                    # B, T, lengths: L = 256 is shorter than the largest dilation 512, L = 512 equals it
CASE2 = (4, 7, (7, 1, 3, 2))                       # hop 300: L_b = 2100, 300, 900, 600 — no row ends on a tile or a wave boundary
HOP300_SCALES = [3, 4, 5, 5]


def rag_inputs(form, B, T, hop=256):
    """z [B, 1, T hop], mel [B, 80, T] UNPADDED, coarse pitch [B, T] or None."""
    return ref.make_inputs(B, T, 7000 + 10 * B + T, 0, form == 'pitch', hop=hop)


def edge(a, n=None):
    """The first n frames of a [.., T] array, edge-padded by the window: what a caller of the padded entry builds for a row alone."""
    if a is None:
        return None
    a = a if n is None else a[..., :n]
    return np.pad(a, ((0, 0),) * (a.ndim - 1) + ((W, W),), 'edge')


class RGen(Gen):
    def ragged_dev(self, z, mel, p, lengths, out=None, seed=0):
        B, T = mel.shape[0], mel.shape[2]
        out = torch.full((B, 1, T * self.hop), float('nan'), device='cuda') if out is None else out
        lens = lengths if isinstance(lengths, Array) else (c_int32 * B)(*lengths)
        _lib.check(self.lib.bsg_pwg_forward_ragged(self.h, _lib.ptr(z), _lib.ptr(mel), _lib.ptr(p), lens, _lib.ptr(out), B, T, seed,
                                                   _lib.stream_ptr()), 'bsg_pwg_forward_ragged')
        return out

    def ragged(self, z, mel, p, lengths, seed=0):
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dt)
        return self.ragged_dev(dev(z, torch.float32), dev(mel, torch.float32), dev(p, torch.int64), lengths, seed=seed).cpu().numpy()

    def lone(self, z, mel, p, b, n):
        """Row b alone through the PADDED entry: B = 1, T = n on the row's own edge-padded mel and pitch."""
        return self.run(z[b:b + 1, :, :n * self.hop], edge(mel[b:b + 1], n), None if p is None else edge(p[b:b + 1], n))[0, 0]

    def tiles(self):
        return self.lib.bsg_pwg_last_tiles(self.h)


@pytest.fixture(params=FORMS)
def gen(request):
    g = RGen(request.param)
    yield g
    torch.cuda.synchronize()
    g.close()


@functools.lru_cache(maxsize=None)
def hop300():
    """(folded weights, generator params) of the small hop-300 generator: 6 layers in 2 stacks, formula weights of seed 23."""
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    q = ref.params(False, layers=6, stacks=2, upsample_params={'upsample_scales': HOP300_SCALES})
    spec = OrderedDict((k, tuple(v.shape)) for k, v in ParallelWaveGANGenerator(**q).state_dict().items())
    folded = ref.fold({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 23).items()})
    return folded, q


def hop300_gen():
    cfg = ref.base_cfg()
    cfg.layers, cfg.stacks, cfg.hop_size = 6, 2, 300
    for i, sc in enumerate(HOP300_SCALES):
        cfg.upsample_scales[i] = sc
    return RGen('plain', hop300()[0], cfg, hop=300)


@functools.lru_cache(maxsize=None)
def rows64(which):
    """which: 'plain' / 'pitch' (CASE1) or 'hop300' (CASE2) -> ([want float64 per row], bound of the weight set).  On the CPU, before any
    kernel of the set runs."""
    if which == 'hop300':
        (B, T, lens), form, hop = CASE2, 'plain', 300
        sd, q = hop300()
    else:
        (B, T, lens), form, hop = CASE1, which, 256
        sd, q = weights(which)[1], ref.params(which == 'pitch')
    z, mel, p = rag_inputs(form, B, T, hop)
    wants, e32 = [], 0.0
    for b, n in enumerate(lens):
        args = (z[b:b + 1, :, :n * hop], edge(mel[b:b + 1], n), None if p is None else edge(p[b:b + 1], n), q)
        want = ref.forward(sd, *args, torch.float64)[0, 0]
        e = float(np.abs(ref.forward(sd, *args, torch.float32)[0, 0] - want).max())
        print(f'[cpu] {which} row {b} ({n} frames): err_fp32 {e:.3e}', flush=True)
        wants.append(want)
        e32 = max(e32, e)
    return wants, 4.0 * e32


def check_rows_equal_the_lone_calls(g, z, mel, p, lens, rows=None):
    got = g.ragged(z, mel, p, lens)
    tiles = g.tiles()
    for b in (range(len(lens)) if rows is None else rows):
        n = lens[b] * g.hop
        assert np.array_equal(got[b, 0, :n], g.lone(z, mel, p, b, lens[b])), (b, lens[b])
    for b, nb in enumerate(lens):
        assert np.all(got[b, 0, nb * g.hop:] == 0.0), b
    return got, tiles


def test_rows_equal_the_lone_call_bit_for_bit(gen):
    B, T, lens = CASE1
    _, tiles = check_rows_equal_the_lone_calls(gen, *rag_inputs(gen.form, B, T), lens)
    assert tiles == sum(lens)                                   # hop = 256: one tile per frame
    z, mel, p = rag_inputs(gen.form, 1, 9)
    check_rows_equal_the_lone_calls(gen, z, mel, p, (4,))
    # all lengths = T: the padded call on the edge-padded batch, and its tile count
    z, mel, p = rag_inputs(gen.form, 8, 33)
    got = gen.ragged(z, mel, p, (33,) * 8)
    assert gen.tiles() == 8 * 33
    assert np.array_equal(got, gen.run(z, edge(mel), edge(p)))
    assert gen.tiles() == 8 * 33


def test_partial_tiles_and_waves_with_a_hop_of_300():
    B, T, lens = CASE2
    g = hop300_gen()
    try:
        _, tiles = check_rows_equal_the_lone_calls(g, *rag_inputs('plain', B, T, 300), lens)
        assert tiles == 9 + 2 + 4 + 3
    finally:
        torch.cuda.synchronize()
        g.close()


@pytest.mark.parametrize('which', ['plain', 'pitch', 'hop300'])
def test_rows_against_float64(which):
    wants, bd = rows64(which)                                   # before the kernel runs
    (B, T, lens), form, hop = (CASE2, 'plain', 300) if which == 'hop300' else (CASE1, which, 256)
    g = hop300_gen() if which == 'hop300' else RGen(which)
    try:
        got = g.ragged(*rag_inputs(form, B, T, hop), lens)
    finally:
        torch.cuda.synchronize()
        g.close()
    bad, worst = [], 0.0
    for b, n in enumerate(lens):
        want = wants[b]
        err, scale = float(np.abs(got[b, 0, :n * hop] - want).max()), max(1.0, float(np.abs(want).max()))
        worst = max(worst, err / scale)
        print(f'{which} row {b} ({n} frames): err {err:.3e} (allowed {bd * scale:.3e}, max |want| {np.abs(want).max():.3f})')
        if not err <= bd * scale:
            bad.append((b, n, err, bd * scale))
    print(f'{which}: bound {bd:.3e} x max(1, max |want|); largest kernel error / max(1, max |want|) = {worst:.3e}')
    assert not bad, bad


def test_nothing_at_or_beyond_a_rows_end_is_read(gen):
    B, T, lens = CASE1
    z, mel, p = rag_inputs(gen.form, B, T)
    clean = gen.ragged(z, mel, p, lens)
    z, mel = z.copy(), mel.copy()
    p = None if p is None else p.copy()
    for b, n in enumerate(lens):
        z[b, :, n * 256:] = np.nan
        mel[b, :, n:] = np.nan
        if p is not None:
            p[b, n:] = np.where(np.arange(T - n) % 2 == 0, -7, 10 ** 6)
    zl, ml, pl = rag_inputs(gen.form, 8, 33)
    gen.run(zl, edge(ml), edge(pl))                              # a long call first: its NaN-free leftovers, then NaN bytes
    gen.poison()
    got = gen.ragged(z, mel, p, lens)
    assert np.isfinite(got).all() and np.array_equal(got, clean)


def test_more_live_tiles_than_compute_units(gen):
    """The persistent workgroups wrap around the live tiles: 355 k of them on a device of fewer compute units (k = 1 on 256)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = 1 + cus // 355
    B, T = 8, 64 * k
    lens = tuple(n * k for n in (64, 1, 63, 33, 64, 2, 64, 64))
    assert sum(lens) == 355 * k and 355 * k > cus
    _, tiles = check_rows_equal_the_lone_calls(gen, *rag_inputs(gen.form, B, T), lens, rows=(1, 3, 7))
    assert tiles == 355 * k and B * T == 512 * k


def test_captured_ragged_forward_replays_its_lengths(gen):
    """One stream, a chain of kernel nodes: no parallel branches.  The workspaces and the lengths array are sized by the eager call; the
    counts travel in kernel arguments, so the replay does not look at the host array again."""
    B, T, lens = CASE1
    z, mel, p = rag_inputs(gen.form, B, T)
    dz, dm = torch.from_numpy(z).cuda(), torch.from_numpy(mel).cuda()
    dp = None if p is None else torch.from_numpy(p).cuda()
    host = (c_int32 * B)(*lens)
    eager = gen.ragged_dev(dz, dm, dp, host).clone()
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gen.ragged_dev(dz, dm, dp, host, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for b in range(B):
        host[b] = T
    for _ in range(2):
        gen.poison()
        out.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_drawn_noise_keeps_the_padded_calls_index(gen):
    """z == NULL: row b sees element b T hop + t of stream 0x505747, as in the padded call at (B, T) — bit for bit the call fed with the
    device's stream, and the host's stream (synth.philox_normal) fed in to 5e-6."""
    B, T, lens = CASE1
    seed, n = 20240607, B * T * 256                             # a multiple of 4
    _, mel, p = rag_inputs(gen.form, B, T)
    drawn = gen.ragged(None, mel, p, lens, seed=seed)
    assert gen.path() == 'ragged ' + expected_path(gen.form, supplied_z=False)
    zdev = torch.empty(B, 1, T * 256, device='cuda')
    _lib.check(gen.lib.bsg_philox_normal(_lib.ptr(zdev), n, seed, PHILOX_STREAM, 0, _lib.stream_ptr()), 'bsg_philox_normal')
    assert np.array_equal(drawn, gen.ragged(zdev.cpu().numpy(), mel, p, lens))
    fed = gen.ragged(synth.philox_normal(seed, PHILOX_STREAM, n).reshape(B, 1, T * 256), mel, p, lens)
    diff = float(np.abs(drawn - fed).max())
    print(f'{gen.form}: ragged, drawn on the device vs the host stream fed in: {diff:.3e}')
    assert diff <= 5e-6
    for b, nb in enumerate(lens):
        assert np.all(drawn[b, 0, nb * 256:] == 0.0)
    assert float(np.abs(drawn - gen.ragged(None, mel, p, lens, seed=seed + 1)).max()) > 1e-3


def test_last_path_is_ragged_plus_the_padded_tokens(gen):
    B, T, lens = CASE1
    gen.ragged(*rag_inputs(gen.form, B, T), lens)
    assert gen.path() == 'ragged ' + expected_path(gen.form)
    z, mel, p = rag_inputs(gen.form, 1, 2)
    gen.run(z, edge(mel), edge(p))
    assert gen.path() == expected_path(gen.form)


@pytest.mark.parametrize('form', FORMS)
def test_spec2wav_batch_end_to_end(tmp_path, form):
    """PWG().spec2wav_batch from a synthetic checkpoint directory: three items of 5, 1 and 9 frames in one ragged forward, each bit for bit
    the waveform spec2wav makes of it alone; through ParallelWaveGANGenerator.forward_ragged, whose last_tiles / last_path are checked too."""
    import yaml
    from bisinger_amd import vocoders
    from bisinger_amd.hparams import hparams
    from tests.util import use_config
    w, _ = weights(form)
    gp = ref.params(form == 'pitch')
    rs = np.random.RandomState(45)
    frames = [5, 1, 9]
    mels = [(rs.standard_normal((T, 80)) * 1.5 - 3.0).astype(np.float32) for T in frames]
    f0s = [rs.uniform(80, 600, size=T).astype(np.float32) for T in frames] if form == 'pitch' else None
    if f0s is not None:
        f0s[2][4:6] = 0
    zs = [rs.standard_normal(T * 256).astype(np.float32) for T in frames]
    use_config()
    try:
        d = tmp_path / 'voc'
        d.mkdir()
        yaml.safe_dump({'generator_params': gp, 'hop_size': 256, 'format': 'hdf5'}, open(d / 'config.yaml', 'w'))
        torch.save({'state_dict': {'model_gen.' + k: v for k, v in w.items()}}, d / 'model_ckpt_steps_3.ckpt')
        hparams['vocoder_ckpt'] = str(d)
        voc = vocoders.get_vocoder_cls({'vocoder': 'pwg'})()
        got = voc.spec2wav_batch(mels, f0s=f0s, zs=zs)
        assert voc.model.last_tiles() == sum(frames) and voc.model.last_path() == 'ragged ' + expected_path(form)
        assert len(got) == 3
        for i, T in enumerate(frames):
            kw = {} if f0s is None else {'f0': f0s[i]}
            want = voc.spec2wav(mels[i], z=zs[i], **kw)
            assert got[i].shape == want.shape == (T * 256,) and np.array_equal(got[i], want), i
        assert voc.model.last_tiles() == 9
        # without zs the noise is drawn on the device: reproducible from the seed, different for another seed
        a, b, c = (voc.spec2wav_batch(mels, f0s=f0s, seed=s) for s in (5, 5, 6))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and float(np.abs(a[2] - c[2]).max()) > 1e-3
        with pytest.raises(_lib.BsgError, match=r'lengths\[1\]=0 outside 1\.\.T=5'):
            voc.model.forward_ragged(None, torch.zeros(2, 80, 5), None if f0s is None else torch.ones(2, 5, dtype=torch.int64),
                                     lengths=[5, 0], seed=1)
    finally:
        use_config()
