"""GPU: the vocoder_denoise_c post-filter (csrc/wavden.hip, bsg_wavden_*) through the C ABI against its float64 restatement
(tests/wavden_ref.py; pinned against torch.stft / torch.istft in tests/test_wavden_cpu.py — librosa is not installed, so there is no golden
of the reference's own run).

Tolerance: ONE number per (fft_size, hop_size, win_size): 4 x the largest err_fp32 over that triple's cases, x max(1, max |want|) of the case,
where err_fp32 = max-abs of the restatement evaluated in float32 against the same in float64 (computed here, on the CPU, by `bound()`).
Four is the margin the project's other kernels have over the fp32 oracle (test_gpu_hifigan_shapes.py) and covers a different summation
order in a 512- or 1024-term sum.  The bounds were computed on the CPU before the kernel ran; beside them the kernel's largest error over
the triple's 104 cases (both amplitudes, all frame counts, all v), divided by max(1, max |want|) like the bound:
    (512, 128, 512)    largest err_fp32 1.273e-06 -> bound 5.093e-06 x max(1, max |want|)    kernel 1.723e-06
    (1024, 256, 1024)  largest err_fp32 1.361e-06 -> bound 5.443e-06 x max(1, max |want|)    kernel 2.261e-06
    (1024, 256, 800)   largest err_fp32 1.467e-06 -> bound 5.869e-06 x max(1, max |want|)    kernel 2.289e-06
The largest err_fp32 is always a case at 10 x amplitude (max |want| ~ 4); the kernel's largest error is too (9.4e-06 absolute where 2.4e-05
is allowed).  v = 50 zeroes every bin only where no bin reaches 50 — (512, 128, 512) at amplitude 0.36, whose peak |S| is 38 — and there
the output must be exactly 0; at n_fft = 1024 (peak 77) or 10 x amplitude the case is an ordinary one."""
import ctypes
import functools
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

from bisinger_amd import _lib
from tests import wavden_ref as ref
from tests.test_gpu_infer import _item, workdir  # noqa: F401  (the synthetic checkpoint directory of the inference tests)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TRIPLES = [(512, 128, 512), (1024, 256, 1024), (1024, 256, 800)]
FRAMES = [1, 2, 3, 4, 5, 28, 29, 30, 31, 32, 33, 1000, 3001]      # a workgroup owns 29 output hops: 29 +- 1 beside the issue's 32 +- 1
VS = [1e-3, 0.1, 0.5, 50.0]
AMPS = [1.0, 10.0]
EINVAL = -22


@functools.lru_cache(maxsize=None)
def cases(triple):
    """[(amp, T, v, want float64, err_fp32)] of one parameter triple."""
    n_fft, hop, win = triple
    out = []
    for amp in AMPS:
        for T in FRAMES:
            y = ref.make_wave(T * hop, amp)
            for v in VS:
                want = ref.denoise(y, v, n_fft, hop, win)
                e32 = float(np.abs(ref.denoise(y, v, n_fft, hop, win, np.float32) - want).max())
                out.append((amp, T, v, want, e32))
    return out


def bound(triple):
    return 4.0 * max(c[4] for c in cases(triple))


class Filter:
    def __init__(self, triple):
        self.lib = _lib.load()
        self.h = c_void_p()
        self.triple = triple
        _lib.check(self.lib.bsg_wavden_create(byref(self.h), *triple, _lib.stream_ptr()), 'bsg_wavden_create')

    def run_dev(self, x, lengths, v, out=None):
        """x: device [B, stride]; -> device [B, stride]."""
        B, stride = x.shape
        n = (ctypes.c_int32 * B)(*lengths) if lengths is not None else None
        out = torch.full_like(x, float('nan')) if out is None else out
        _lib.check(self.lib.bsg_wavden_forward(self.h, _lib.ptr(x), _lib.ptr(out), n, B, stride, v, _lib.stream_ptr()), 'bsg_wavden_forward')
        return out

    def run(self, y, v, stride=None):
        """One waveform (numpy [L]) alone; -> numpy [stride]."""
        x = torch.from_numpy(np.asarray(y, np.float32))
        if stride is not None and stride > len(y):
            x = torch.cat([x, torch.full((stride - len(y),), float('nan'))])
        out = self.run_dev(x.cuda().view(1, -1), [len(y)], v)
        return out[0].cpu().numpy()

    def close(self):
        self.lib.bsg_wavden_destroy(self.h)


@pytest.fixture(params=TRIPLES, ids=lambda t: '-'.join(map(str, t)))
def flt(request):
    f = Filter(request.param)
    yield f
    torch.cuda.synchronize()
    f.close()


def test_every_case_against_float64(flt):
    """Both amplitudes x 13 frame counts x 4 values of v; the bound of the module docstring, one number per triple."""
    n_fft, hop, win = flt.triple
    bd = bound(flt.triple)
    bad, worst, all_zero = [], 0.0, 0
    for amp, T, v, want, e32 in cases(flt.triple):
        got = flt.run(ref.make_wave(T * hop, amp), v)
        assert got.shape == want.shape
        err = float(np.abs(got - want).max())
        scale = max(1.0, float(np.abs(want).max()))
        worst = max(worst, err / scale)
        print(f'{flt.triple} amp={amp} T={T} v={v}: err {err:.3e} (err_fp32 {e32:.3e}, allowed {bd * scale:.3e}, max |want| {np.abs(want).max():.3f})')
        if not err <= bd * scale:
            bad.append((amp, T, v, err, bd * scale))
        if not np.abs(want).max() > 0:          # the threshold is above every bin: exactly 0, not merely small
            all_zero += 1
            assert not got.any(), (amp, T, v)
    print(f'{flt.triple}: bound {bd:.3e} x max(1, max |want|); largest kernel error / max(1, max |want|) = {worst:.3e}')
    assert not bad, bad
    if flt.triple == (512, 128, 512):
        assert all_zero >= len(FRAMES)          # v = 50 at amplitude 0.36 zeroes everything


def test_batch_rows_are_independent_and_padding_is_never_read(flt):
    """B = 16 rows of U(1 .. 1000) frames in one call: each row bit-identical to the same row filtered alone at B = 1, exactly 0 beyond its
    length; the padding of the input holds NaN bytes."""
    n_fft, hop, win = flt.triple
    rs = np.random.RandomState(1)
    frames = [int(t) for t in rs.randint(1, 1001, size=16)]
    frames[3], frames[7] = 1, 1000
    stride = max(frames) * hop
    x = np.frombuffer(b'\xff' * (16 * stride * 4), dtype=np.float32).reshape(16, stride).copy()
    assert np.isnan(x).all()
    waves = [ref.make_wave(t * hop, 1.0, seed=10 + i) for i, t in enumerate(frames)]
    for i, w in enumerate(waves):
        x[i, :len(w)] = w
    got = flt.run_dev(torch.from_numpy(x).cuda(), [t * hop for t in frames], 0.1).cpu().numpy()
    assert np.isfinite(got).all()
    bd = bound(flt.triple)
    for i, w in enumerate(waves):
        alone = flt.run(w, 0.1)
        assert np.array_equal(got[i, :len(w)], alone), i
        assert not got[i, len(w):].any(), i
        if i < 4:
            want = ref.denoise(w, 0.1, n_fft, hop, win)
            assert float(np.abs(alone - want).max()) <= bd * max(1.0, float(np.abs(want).max()))
    # more rows than one launch carries (64): still every row as if alone
    many = torch.from_numpy(np.stack([ref.make_wave(5 * hop, 1.0, seed=i) for i in range(70)])).cuda()
    lens = [(1 + i % 5) * hop for i in range(70)]
    got = flt.run_dev(many, lens, 0.1).cpu().numpy()
    for i in (0, 63, 64, 69):
        assert np.array_equal(got[i, :lens[i]], flt.run(many[i, :lens[i]].cpu().numpy(), 0.1)) and not got[i, lens[i]:].any()


def test_length_not_a_multiple_of_hop_and_out_of_place(flt):
    n_fft, hop, win = flt.triple
    L = 37 * hop + hop // 3
    y = ref.make_wave(L)
    want = ref.denoise(y, 0.1, n_fft, hop, win)
    got = flt.run(y, 0.1, stride=L + 5)           # 5 NaN samples of padding behind the row
    assert got.shape == (L + 5,) and want.shape == (37 * hop,)
    assert float(np.abs(got[:37 * hop] - want).max()) <= bound(flt.triple) * max(1.0, float(np.abs(want).max()))
    assert not got[37 * hop:].any()               # 0 beyond hop * (L // hop), up to the stride
    short = flt.run(y[:hop - 1], 0.1)             # shorter than one hop: no output frame
    assert short.shape == (hop - 1,) and not short.any()
    # not in place (include/bisinger_hip.h): refused, nothing launched
    x = torch.from_numpy(y).cuda().view(1, -1)
    n = (ctypes.c_int32 * 1)(L)
    assert flt.lib.bsg_wavden_forward(flt.h, _lib.ptr(x), _lib.ptr(x), n, 1, L, 0.1, _lib.stream_ptr()) == EINVAL
    assert 'overlaps' in flt.lib.bsg_last_error().decode()
    assert flt.lib.bsg_wavden_forward(flt.h, _lib.ptr(x), _lib.ptr(x), n, 1, L, -1.0, _lib.stream_ptr()) == EINVAL


def test_captured_launch_replays_bit_identically(flt):
    """One stream, one kernel node: no parallel branches."""
    n_fft, hop, win = flt.triple
    x = torch.from_numpy(np.stack([ref.make_wave(100 * hop, 1.0, seed=s) for s in (3, 4)])).cuda()
    lens = [100 * hop, 61 * hop + 7]
    eager = flt.run_dev(x, lens, 0.1).clone()
    out = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            flt.run_dev(x, lens, 0.1, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_spec2wav_applies_the_filter_on_the_device(tmp_path, sd_spec):
    """HifiGAN.spec2wav with vocoder_denoise_c = 0.1 == the restatement applied to the same wrapper's output at vocoder_denoise_c = 0."""
    import json
    from collections import OrderedDict
    from bisinger_amd import synth, vocoders
    from bisinger_amd.hparams import hparams
    from tests.util import use_config
    cfg = sd_spec['hifigan_v1_json']
    spec = OrderedDict((k, tuple(s)) for k, s in sd_spec['HifiGanGenerator_weight_norm'])
    json.dump(cfg, open(tmp_path / 'config.json', 'w'))
    torch.save({'generator': {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(spec, 7).items()}}, tmp_path / 'generator_v1')
    use_config()
    try:
        hparams['vocoder_ckpt'] = str(tmp_path)
        voc = vocoders.HifiGAN()
        mel = (np.random.RandomState(33).standard_normal((40, 80)) * 1.5 - 3.0).astype(np.float32)
        plain = voc.spec2wav(mel)
        hparams['vocoder_denoise_c'] = 0.1
        got = voc.spec2wav(mel)
        triple = (hparams['fft_size'], hparams['hop_size'], hparams['win_size'])
        assert triple == (512, 128, 512) and plain.shape == got.shape == (40 * 256,)
        want = ref.denoise(plain, 0.1, *triple)
        err = float(np.abs(got - want).max())
        print(f'spec2wav: err {err:.3e}, max |want| {np.abs(want).max():.3f}, the filter moved samples by up to {np.abs(want - plain).max():.3f}')
        assert err <= bound(triple) * max(1.0, float(np.abs(want).max()))
        assert float(np.abs(want - plain).max()) > 1e-3
        # the module-level entry with the reference's signature: numpy in, numpy out
        assert np.array_equal(vocoders.denoise(plain, v=0.1), got)
    finally:
        use_config()


def test_forward_batch_applies_the_filter_per_row(workdir):  # noqa: F811
    """forward_batch(denoise_c=0.1) == forward_batch() followed by the restatement on every returned row."""
    from bisinger_amd.hparams import hparams, set_hparams
    from bisinger_amd.infer import DiffSingerE2EInfer
    set_hparams('exp.yaml', exp_name='exp_diff_e2e', print_hparams=False, hparams_str='seed=4321')
    infer = DiffSingerE2EInfer(hparams)
    items = [infer.preprocess_input(_item(n, s), 'phoneme') for n, s in ((9, 1), (6, 2), (11, 3))]
    plain = infer.forward_batch(items, seed=77)
    got = infer.forward_batch(items, seed=77, denoise_c=0.1)
    triple = (hparams['fft_size'], hparams['hop_size'], hparams['win_size'])
    assert triple == (512, 128, 512)
    for p, g in zip(plain, got):
        want = ref.denoise(p, 0.1, *triple)
        assert g.shape == p.shape == want.shape
        err = float(np.abs(g - want).max())
        print(f'forward_batch row of {len(p)} samples: err {err:.3e}, max |want| {np.abs(want).max():.3f}')
        assert err <= bound(triple) * max(1.0, float(np.abs(want).max()))
    assert max(float(np.abs(g - p).max()) for p, g in zip(plain, got)) > 1e-3
