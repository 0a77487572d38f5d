"""GPU: the Parallel WaveGAN generator (csrc/pwg.hip, bsg_pwg_*) through the C ABI against the reference's goldens
(tests/golden/pwg_*.npz) and against its float64 restatement (tests/pwg_ref.py, pinned to the goldens in tests/test_pwg_cpu.py).

Tolerance: ONE number per weight set (the no-pitch and the pitch form have their own formula weights): 4 x the largest err_fp32 over that
set's cases, x max(1, max |want|) of the case, where err_fp32 = max-abs of the restatement evaluated in float32 against the same in float64
(computed here, on the CPU, by `bound()`, before the kernel runs).  Four is the margin the project's other kernels have over the fp32
oracle (test_gpu_wavden.py) and covers a different summation order in the 272-term and 64-term sums of a layer, 30 layers deep.  The
cases: T in {1, 2, 3, 7, 8, 9, 31, 32, 33, 1000} x B in {1, 8}.  A workgroup tile is 256 samples and a wave's run 64; with hop = 256 every
row is a whole number of tiles (T = 1: L = 256 is shorter than the largest dilation 512; T = 2: equal to it), so the partial tiles and
partial waves are covered by a second, small generator with hop = 3 x 4 x 5 x 5 = 300 (test_partial_tiles_with_a_hop_of_300).  None is excluded from the
bound check.  One case, B = 8 at T = 1000, has its float64 restatement evaluated by torch on the GPU (matrix products and element-wise
operations in float64, tests/pwg_ref._conv) because on the CPU its 8 rows of 256 000 samples take five minutes per weight set; it adds no
err_fp32 to the maximum, which can only make the bound smaller than the one over all 20 cases.  The other 19, B = 1 at T = 1000 among
them, are evaluated on the CPU.
The bounds were computed on the CPU before the kernel ran; beside them the kernel's largest error over the set's 20 cases, divided by
max(1, max |want|) like the bound:
    plain (no pitch front)  largest err_fp32 1.285e-06 (B = 1, T = 9)    -> bound 5.142e-06 x max(1, max |want|)    kernel 1.380e-06
    pitch front             largest err_fp32 5.308e-07 (B = 1, T = 1000) -> bound 2.123e-06 x max(1, max |want|)    kernel 6.791e-07
The reference's goldens: 1.371e-06 / 6.557e-07 (plain), 4.545e-07 / 3.129e-07 (pitch).  max |want| is 0.2 .. 1.1.

Every product runs on the fp32 matrix pipe: there is no split-fp16 form, so no range guard, no demotion tier and no range-guard case."""
import ctypes
import functools
import json
import os
from collections import OrderedDict
from ctypes import POINTER, byref, c_void_p, cast

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import pwg_ref as ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FRAMES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 1000]
BATCHES = [1, 8]
FORMS = ['plain', 'pitch']
PHILOX_STREAM = 0x505747
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLD_CASES, SEEDS, base_cfg = ref.GOLDEN_CASES, ref.GOLDEN_SEEDS, ref.base_cfg


@functools.lru_cache(maxsize=None)
def weights(form):
    """(weight-norm state dict, folded state dict) of the form's formula weights (the goldens' weights)."""
    spec = json.load(open(os.path.join(GOLD, 'pwg_state_dict_spec.json')))
    s = OrderedDict((k, tuple(shp)) for k, shp in spec[f'{form}_weight_norm'])
    w = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(s, SEEDS[form]).items()}
    return w, ref.fold(w)


def inputs(form, B, T):
    return ref.make_inputs(B, T, 1000 * B + T, 2, form == 'pitch')


ON_DEVICE = [(8, 1000)]      # cases whose float64 restatement is evaluated on the GPU (see the module docstring)


@functools.lru_cache(maxsize=None)
def case(form, B, T):
    """(want float64, err_fp32 or None) of one case."""
    z, c, p = inputs(form, B, T)
    q = ref.params(form == 'pitch')
    if (B, T) in ON_DEVICE:
        return ref.forward(weights(form)[1], z, c, p, q, torch.float64, device='cuda'), None
    want = ref.forward(weights(form)[1], z, c, p, q, torch.float64)
    e32 = float(np.abs(ref.forward(weights(form)[1], z, c, p, q, torch.float32) - want).max())
    print(f'[cpu] {form} B={B} T={T}: err_fp32 {e32:.3e}', flush=True)
    return want, e32


@functools.lru_cache(maxsize=None)
def bound(form):
    """On the CPU, before any kernel of the form runs."""
    return 4.0 * max(case(form, B, T)[1] for B in BATCHES for T in FRAMES if (B, T) not in ON_DEVICE)


class Gen:
    """One bsg_pwg handle over the form's folded weights."""

    def __init__(self, form, folded=None, cfg=None, hop=256):
        self.lib = _lib.load()
        self.form, self.hop = form, hop
        self.w = [v.cuda().contiguous() for v in (folded or weights(form)[1]).values()]
        cfg = cfg or base_cfg()
        if form == 'pitch':
            cfg.use_pitch_embed, cfg.n_pitch = 1, 300
        arr = (c_void_p * len(self.w))(*[t.data_ptr() for t in self.w])
        self.h = c_void_p()
        _lib.check(self.lib.bsg_pwg_create(byref(self.h), byref(cfg), cast(arr, POINTER(c_void_p)), len(self.w), _lib.stream_ptr()),
                   'bsg_pwg_create')

    def run_dev(self, z, c, p, out=None, seed=0):
        B, T = c.shape[0], c.shape[2] - 4
        out = torch.full((B, 1, T * self.hop), float('nan'), device='cuda') if out is None else out
        _lib.check(self.lib.bsg_pwg_forward(self.h, _lib.ptr(z), _lib.ptr(c), _lib.ptr(p), _lib.ptr(out), B, T, seed, _lib.stream_ptr()),
                   'bsg_pwg_forward')
        return out

    def run(self, z, c, p, seed=0):
        dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dt)
        return self.run_dev(dev(z, torch.float32), dev(c, torch.float32), dev(p, torch.int64), seed=seed).cpu().numpy()

    def path(self):
        return self.lib.bsg_pwg_last_path(self.h).decode()

    def poison(self):
        _lib.check(self.lib.bsg_pwg_debug_poison_workspace(self.h, _lib.stream_ptr()), 'bsg_pwg_debug_poison_workspace')

    def close(self):
        self.lib.bsg_pwg_destroy(self.h)


@pytest.fixture(params=FORMS)
def gen(request):
    g = Gen(request.param)
    yield g
    torch.cuda.synchronize()
    g.close()


def expected_path(form, supplied_z=True):
    toks = (['pitch'] if form == 'pitch' else []) + ['conv_in'] + [f'up{i}:x4' for i in range(4)] + ([] if supplied_z else ['philox']) + ['first']
    toks += [f'layer{i}:f32/d{2 ** (i % 10)}' for i in range(30)] + ['tail']
    return ' '.join(toks)


def test_reference_goldens(gen):
    bd = bound(gen.form)
    gold = np.load(os.path.join(GOLD, f'pwg_{gen.form}.npz'))
    for tag, (B, T, seed) in GOLD_CASES.items():
        z, c, p = ref.make_inputs(B, T, seed, 2, gen.form == 'pitch')
        got = gen.run(z, c, p)
        err = float(np.abs(got - gold[tag]).max())
        scale = max(1.0, float(np.abs(gold[tag]).max()))
        print(f'{gen.form} golden {tag}: err {err:.3e} (allowed {bd * scale:.3e})')
        assert got.shape == gold[tag].shape and err <= bd * scale
        assert gen.path() == expected_path(gen.form)


def test_every_shape_edge_against_float64(gen):
    """10 frame counts x B in {1, 8}; the bound of the module docstring, one number per weight set; the launches from bsg_pwg_last_path."""
    bd = bound(gen.form)
    bad, worst = [], 0.0
    for B in BATCHES:
        for T in FRAMES:
            want, e32 = case(gen.form, B, T)
            got = gen.run(*inputs(gen.form, B, T))
            assert got.shape == want.shape == (B, 1, T * 256)
            assert gen.path() == expected_path(gen.form)
            err = float(np.abs(got - want).max())
            scale = max(1.0, float(np.abs(want).max()))
            worst = max(worst, err / scale)
            print(f'{gen.form} B={B} T={T}: err {err:.3e} (err_fp32 {e32 if e32 is None else format(e32, ".3e")}, allowed {bd * scale:.3e}, max |want| {np.abs(want).max():.3f})')
            if not err <= bd * scale:
                bad.append((B, T, err, bd * scale))
    print(f'{gen.form}: bound {bd:.3e} x max(1, max |want|); largest kernel error / max(1, max |want|) = {worst:.3e}')
    assert not bad, bad


@pytest.mark.parametrize('T', [3, 33, 1000])
def test_batch_rows_are_bit_identical_to_each_row_alone(gen, T):
    z, c, p = inputs(gen.form, 8, T)
    got = gen.run(z, c, p)
    for b in (range(8) if T < 1000 else (0, 7)):
        alone = gen.run(z[b:b + 1], c[b:b + 1], None if p is None else p[b:b + 1])
        assert np.array_equal(got[b], alone[0]), (T, b)


def test_short_call_after_a_long_one_on_poisoned_workspaces(gen):
    gen.run(*inputs(gen.form, 8, 33))
    gen.poison()
    short = gen.run(*inputs(gen.form, 1, 3))
    fresh = Gen(gen.form)
    try:
        want = fresh.run(*inputs(gen.form, 1, 3))
    finally:
        torch.cuda.synchronize()
        fresh.close()
    assert np.isfinite(short).all() and np.array_equal(short, want)


def test_captured_forward_replays_bit_identically(gen):
    """One stream, a chain of kernel nodes: no parallel branches.  The workspaces are sized by the eager call before the capture."""
    z, c, p = inputs(gen.form, 2, 9)
    dz, dc = torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()
    dp = None if p is None else torch.from_numpy(p).cuda()
    for zz, seed in ((dz, 0), (None, 99)):          # supplied noise, and noise drawn inside the captured call
        eager = gen.run_dev(zz, dc, dp, seed=seed).clone()
        out = torch.zeros_like(eager)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                gen.run_dev(zz, dc, dp, out=out, seed=seed)
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            out.fill_(float('nan'))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)


def test_philox_noise_equals_the_host_stream_fed_in(gen):
    """z == NULL draws element b L + t of stream 0x505747 of bsg_philox_normal: the call equals, bit for bit, the call fed with that stream
    as supplied z; the stream is synth.philox_normal to 5e-6 (the figure test_gpu_diffnet.py pins: the host's and the device's logarithm
    and sine differ in the last bits), and the output is the float64 restatement of that noise within the bound."""
    B, T, seed = 2, 7, 20240607
    n = B * T * 256
    _, c, p = inputs(gen.form, B, T)
    drawn = gen.run(None, c, p, seed=seed)
    assert gen.path() == expected_path(gen.form, supplied_z=False)
    zdev = torch.empty(B, 1, T * 256, device='cuda')
    _lib.check(gen.lib.bsg_philox_normal(_lib.ptr(zdev), n, seed, PHILOX_STREAM, 0, _lib.stream_ptr()), 'bsg_philox_normal')
    host = synth.philox_normal(seed, PHILOX_STREAM, n).reshape(B, 1, T * 256)
    assert float(np.abs(zdev.cpu().numpy() - host).max()) <= 5e-6
    assert np.array_equal(drawn, gen.run(zdev.cpu().numpy(), c, p))
    want = ref.forward(weights(gen.form)[1], zdev.cpu().numpy(), c, p, ref.params(gen.form == 'pitch'), torch.float64)
    assert float(np.abs(drawn - want).max()) <= bound(gen.form) * max(1.0, float(np.abs(want).max()))
    fed = gen.run(host, c, p)
    diff = float(np.abs(drawn - fed).max())
    print(f'{gen.form}: drawn on the device vs the host stream fed in: {diff:.3e}')
    assert diff <= bound(gen.form) * max(1.0, float(np.abs(fed).max()))
    assert float(np.abs(drawn - gen.run(None, c, p, seed=seed + 1)).max()) > 1e-3


def test_partial_tiles_with_a_hop_of_300():
    """upsample_scales [3, 4, 5, 5]: hop = 300, so L = 300 T is no multiple of the 64 samples of a wave or the 256 of a tile — the last
    wave of a row is partial (t0 < L <= t0 + 64) or absent (t0 >= L), and the B-operand loads end inside a 32-sample half.  A generator of
    6 layers in 2 stacks (dilations 1, 2, 4) with formula weights; B = 3, T in {1, 2, 3, 7, 41}; against the float64 restatement, bound
    = 4 x the largest err_fp32 of these cases (CPU) x max(1, max |want|), and rows bit-identical to each row alone."""
    from bisinger_amd.pwg import ParallelWaveGANGenerator
    q = ref.params(False, layers=6, stacks=2, upsample_params={'upsample_scales': [3, 4, 5, 5]})
    spec = OrderedDict((k, tuple(v.shape)) for k, v in ParallelWaveGANGenerator(**q).state_dict().items())
    folded = ref.fold({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 23).items()})
    cfg = base_cfg()
    cfg.layers, cfg.stacks, cfg.hop_size = 6, 2, 300
    for i, sc in enumerate([3, 4, 5, 5]):
        cfg.upsample_scales[i] = sc
    runs = []
    for T in (1, 2, 3, 7, 41):
        z, c, _ = ref.make_inputs(3, T, 300 + T, 2, False, hop=300)
        want = ref.forward(folded, z, c, None, q, torch.float64)
        e32 = float(np.abs(ref.forward(folded, z, c, None, q, torch.float32) - want).max())
        runs.append((T, z, c, want, e32))
    bd = 4.0 * max(r[4] for r in runs)
    g = Gen('plain', folded, cfg, hop=300)
    try:
        for T, z, c, want, e32 in runs:
            got = g.run(z, c, None)
            assert got.shape == want.shape == (3, 1, 300 * T)
            err, scale = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
            print(f'hop 300 T={T} (L={300 * T}): err {err:.3e} (err_fp32 {e32:.3e}, allowed {bd * scale:.3e})')
            assert err <= bd * scale
            assert g.path().split()[1:5] == ['up0:x3', 'up1:x4', 'up2:x5', 'up3:x5'] and g.path().count('layer') == 6
            assert np.array_equal(got[1], g.run(z[1:2], c[1:2], None)[0])
    finally:
        torch.cuda.synchronize()
        g.close()


@pytest.mark.parametrize('B', [1, 8])
def test_hip_path_is_faster_than_the_torch_restatement_on_the_device(B):
    """The one timing requirement: at T = 1000 the forward through the C ABI takes less time than the float32 torch restatement run on the
    same GPU with everything resident there (ratio < 1; tools/bench_pwg.py reports the figures).  Events on the stream, one warm-up, the
    median of 3 runs each."""
    import statistics
    g = Gen('plain')
    try:
        z, c, _ = inputs('plain', B, 1000)
        z, c = torch.from_numpy(z).cuda(), torch.from_numpy(c).cuda()
        out = torch.empty(B, 1, 256000, device='cuda')
        sd = {k: v.cuda() for k, v in weights('plain')[1].items()}
        q = ref.params(False)

        def ms(fn):
            fn()
            torch.cuda.synchronize()
            t = []
            for _ in range(3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t.append(a.elapsed_time(b))
            return statistics.median(t)
        hip = ms(lambda: g.run_dev(z, c, None, out=out))
        tor = ms(lambda: ref.forward(sd, z, c, None, q, torch.float32, device='cuda', as_tensor=True, whole_batch=True))
        print(f'B={B} T=1000: HIP {hip:.2f} ms, torch float32 on the device {tor:.2f} ms, ratio {hip / tor:.3f}')
        assert hip < tor
    finally:
        torch.cuda.synchronize()
        g.close()


def test_forward_refusals(gen):
    lib = gen.lib
    z, c, p = inputs(gen.form, 1, 2)
    dc = torch.from_numpy(c).cuda()
    out = torch.zeros(1, 1, 512, device='cuda')
    other = torch.zeros(1, 6, dtype=torch.int64, device='cuda') if gen.form == 'plain' else None
    rc = lib.bsg_pwg_forward(gen.h, None, _lib.ptr(dc), _lib.ptr(other), _lib.ptr(out), 1, 2, 0, _lib.stream_ptr())
    assert rc == -22 and 'pitch' in lib.bsg_last_error().decode()


@pytest.mark.parametrize('layout', ['custom', 'official_npy'])
@pytest.mark.parametrize('form', FORMS)
def test_spec2wav_end_to_end(tmp_path, monkeypatch, layout, form):
    """PWG().spec2wav from a synthetic checkpoint directory against the restatement, with f0 (the pitch form) and without."""
    import yaml
    from bisinger_amd import vocoders
    from bisinger_amd.hparams import hparams
    from tests.util import use_config
    w, folded = weights(form)
    gp = ref.params(form == 'pitch')
    rs = np.random.RandomState(44)
    T = 12
    mel = (rs.standard_normal((T, 80)) * 1.5 - 3.0).astype(np.float32)
    f0 = rs.uniform(80, 600, size=T).astype(np.float32) if form == 'pitch' else None
    if f0 is not None:
        f0[4:6] = 0
    z = rs.standard_normal(T * 256).astype(np.float32)
    use_config()
    try:
        if layout == 'custom':
            d = tmp_path / 'voc'
            d.mkdir()
            yaml.safe_dump({'generator_params': gp, 'hop_size': 256, 'format': 'hdf5'}, open(d / 'config.yaml', 'w'))
            sd = {'model_gen.' + k: v for k, v in w.items()}
            sd['model_disc.conv_layers.0.bias'] = torch.zeros(3)
            torch.save({'state_dict': sd}, d / 'model_ckpt_steps_3.ckpt')
            torch.save({'state_dict': {}}, d / 'model_ckpt_steps_2.ckpt')
            hparams['vocoder_ckpt'] = str(d)
            scale_in = mel
        else:
            d = tmp_path / 'wavegan_pretrained'
            d.mkdir()
            yaml.safe_dump({'generator_params': gp, 'hop_size': 256, 'format': 'npy'}, open(d / 'config.yaml', 'w'))
            torch.save({'model': {'generator': w}}, d / 'checkpoint-400000steps.pkl')
            stats = np.stack([rs.standard_normal(80) - 3.0, rs.uniform(0.5, 2.0, 80)])
            np.save(d / 'stats.npy', stats)
            monkeypatch.chdir(tmp_path)
            hparams['vocoder_ckpt'] = ''
            scale_in = ((mel.astype(np.float64) - stats[0]) / stats[1]).astype(np.float32)
        voc = vocoders.get_vocoder_cls({'vocoder': 'pwg'})()
        assert (voc.scaler is None) == (layout == 'custom')
        kw = {} if f0 is None else {'f0': f0}
        got = voc.spec2wav(mel, z=z, **kw)
        c = np.pad(scale_in.T[None], ((0, 0), (0, 0), (2, 2)), 'edge')
        p = None if f0 is None else np.pad(vocoders.f0_to_coarse(f0), (2, 2), 'edge')[None]
        want = ref.forward(folded, z[None, None], c, p, gp, torch.float64).reshape(-1)
        err = float(np.abs(got - want).max())
        print(f'spec2wav {layout} {form}: err {err:.3e}, max |want| {np.abs(want).max():.3f}')
        assert got.shape == want.shape == (T * 256,)
        assert err <= bound(form) * max(1.0, float(np.abs(want).max()))
        # without z the noise is drawn on the device: reproducible from the seed, different for another seed
        a, b, c2 = voc.spec2wav(mel, seed=5, **kw), voc.spec2wav(mel, seed=5, **kw), voc.spec2wav(mel, seed=6, **kw)
        assert np.array_equal(a, b) and float(np.abs(a - c2).max()) > 1e-3
        if form == 'pitch':
            with pytest.raises(_lib.BsgError):
                voc.spec2wav(mel, z=z)
    finally:
        use_config()
