"""GPU: ONE handle of each kind walked through grow -> shrink -> grow again, every step against a FRESH handle that has seen only that step,
and what a stream capture gets when a call would have to grow a workspace (csrc/bsg_ws.h: one table and one grow path for every handle).

tests/test_gpu_rebind.py walks the denoiser's bindings; the "short call after a long one" tests of the other handles only shrink.  What
this file is after is the second growth: a capacity word that no longer matches its buffer after a reallocation, arrival counters that
are not zero behind a regrown key split, a buffer left out of the table that the poison hook then never reaches.  Every such fault shows
as a difference from a handle that has seen nothing but the step's own shape, so the expectation everywhere is outputs bit-equal and
finite, the same launch record where the kind keeps one, and no range event.  Where the kind has a poison hook it runs on the walked
handle before every step.  Models, weights and inputs are those of the files the builders come from.

The capture rule, once per kind on the walked handle while it is warm at the walk's first (smallest) shape only: the walk's second shape
called inside a torch.cuda.graph capture on a side stream is refused (BsgError, REFUSAL below, the handle kind named), the capture ends
normally, and the same shape run eagerly behind it is the walk's second step — bit-equal to the fresh handle's.  For DiffNet the captured
call is a prepare of a larger (B, T): the bound groups, which had no refusal of their own before.

Not walked here: the score tensor of the FFT stacks.  Its group is reached only under the softmax switch, which is read once per process;
the `softmax` set of tests/test_gpu_fs2_shapes.py test_fallback_forms_vs_fp64 grows it step by step against float64 in its child process."""
import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests import pe_cases
from tests.test_gpu_f2_fullsize import nsf  # noqa: F401  (the module-scoped NSF generator fixture of that file)
from tests.test_gpu_fs2_shapes import C, _den_inputs, _den_run, _inputs, _make_fs2, _run, den  # noqa: F401  (den: the FFT denoiser fixture)
from tests.test_gpu_hifigan_ragged import HOP, NH, _f0, _nan_tail
from tests.test_gpu_hifigan_shapes import _mel, _run_guarded, plain  # noqa: F401  (plain: the generator fixture)
from tests.test_gpu_pwg import Gen, inputs as pwg_inputs
from tests.util import load_formula_weights, use_config

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

REFUSAL = 'a workspace has to grow for this shape, which a capturing stream cannot do; run the shape once eagerly before capturing'


def _same(got, want, what):
    """(outputs, launch record or None) of a step on the walked handle against the fresh handle's."""
    (outs_g, path_g), (outs_w, path_w) = got, want
    assert path_g == path_w, (what, path_g, path_w)
    assert len(outs_g) == len(outs_w) and len(outs_g) > 0
    for g, w in zip(outs_g, outs_w):
        g, w = torch.as_tensor(g), torch.as_tensor(w)
        assert torch.isfinite(g).all() and torch.equal(g, w), what


def _refused_under_capture(call, kind):
    """`call()` inside a capture on a side stream raises the refusal, naming the handle kind; the capture then ends normally."""
    marker = torch.zeros(4, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        marker.fill_(1.0)      # (one node of the capture's own: the refused call leaves none)
        with pytest.raises(_lib.BsgError) as e:
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert REFUSAL in str(e.value) and f'{kind}: ' in str(e.value), str(e.value)


def _walk(kind, steps, run, release, poison=None, captured=None):
    """The fresh runs (one handle per step), then the walk on one handle; `captured(step)`: the call of `step` with every input on the device
    already, tried under capture between the first step and the second."""
    fresh = []
    for s in steps:
        release()
        fresh.append(run(s))
    release()
    for i, s in enumerate(steps):
        if poison:
            poison()
        if i == 1:
            _refused_under_capture(captured(s), kind)
        _same(run(s), fresh[i], (kind, i, s))
    release()


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def test_pitch_extractor(sd_spec):
    pe = pe_cases.pitch_extractor(sd_spec).cuda()

    def run(bt):
        before = _lib.range_retries
        r = pe(torch.from_numpy(pe_cases.mel_for(*bt)).cuda())
        assert _lib.range_retries == before and pe.gemm_range_peek() == 0
        return (r['pitch_pred'].cpu(), r['f0_denorm_pred'].cpu()), None

    def captured(bt):
        mel, = _dev(pe_cases.mel_for(*bt))
        return lambda: pe(mel)

    _walk('pitchext', [(1, 5), (3, 65), (1, 4), (3, 129)], run, pe.release, captured=captured)


def test_hifigan_plain(plain):  # noqa: F811
    gen = plain[0]
    # the stage buffers and the GEMM planes grow at (2, 601) and (3, 683), the row lengths at the first ragged call and at B = 5
    steps = [(1, 1, None), (2, 601, None), (1, 2, None), (3, 683, None), (2, 5, [5, 2]), (5, 413, [413, 7, 206, 64, 1])]

    def captured(step):
        mel, = _dev(_mel(step[0], step[1]))
        return lambda: gen(mel)

    _walk('hifigan', steps, lambda s: _plain(gen, *s), gen.release, gen.poison_workspace, captured)


def _plain(gen, B, T, lens):
    mel = _mel(B, T) if lens is None else _nan_tail(_mel(B, T), lens)
    y, path = _run_guarded(gen, torch.from_numpy(mel).cuda(), **({} if lens is None else {'lengths': lens}))
    return (y,), path


def _nsf_inputs(B, T):
    rs = np.random.RandomState(500 * B + T)
    mel = (rs.standard_normal((B, 80, T)) * 1.5 - 3.0).astype(np.float32)
    return mel, _f0(rs, B, T), rs.uniform(0, 1, size=(B, NH)).astype(np.float32), rs.standard_normal((B, T * HOP, NH)).astype(np.float32)


def test_hifigan_nsf(nsf):  # noqa: F811
    gen = nsf[0]

    def run(bt):
        mel, f0, rand_ini, noise = _dev(*_nsf_inputs(*bt))
        y, path = _run_guarded(gen, mel, f0, rand_ini=rand_ini, noise=noise)
        return (y,), path

    def captured(bt):
        mel, f0, rand_ini, noise = _dev(*_nsf_inputs(*bt))
        return lambda: gen(mel, f0, rand_ini=rand_ini, noise=noise)

    # the source buffers grow at (2, 5) and at (2, 601)
    _walk('hifigan', [(1, 1), (2, 5), (1, 2), (2, 601)], run, gen.release, gen.poison_workspace, captured)


def test_fs2_midi():
    m = _make_fs2()
    # the row workspaces grow at 257 and at 511 frames; the key-split partials and their counters at 257 (two splits) and at 511 (four)
    steps = [C(2, 3, 5), C(1, 25, 257), C(1, 4, 10), C(1, 50, 511), C(3, 5, 31)]
    paths = {}

    def run(case):
        got, path = _run(m, _inputs(case))
        paths[case] = path
        return tuple(got.values()), path

    def captured(case):
        d = {k: torch.from_numpy(v).cuda() for k, v in _inputs(case).items()}
        kw = {k: d[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
        return lambda: m(d['txt_tokens'], d['mel2ph'], d['spk_embed'], None, None, None, None, infer=True, **kw)

    _walk('fs2', steps, run, m.release, m.poison_workspace, captured)
    assert 'dec.attn:planes/ks2' in paths[steps[1]].split() and 'dec.attn:planes/ks4' in paths[steps[3]].split(), paths


def test_fft_denoiser(den):  # noqa: F811
    net = den[0]

    def run(bt):
        eps, path = _den_run(net, *bt)
        return (eps,), path

    def captured(bt):
        x, t, cond = _dev(*_den_inputs(*bt))
        return lambda: net(x, t, cond)

    _walk('fftden', [(1, 1), (2, 33), (1, 1), (2, 301)], run, net.release, net.poison_workspace, captured)


def test_pwg_plain():
    state = {'gen': None}

    def release():
        torch.cuda.synchronize()
        if state['gen'] is not None:
            state['gen'].close()
        state['gen'] = None

    def gen():
        if state['gen'] is None:
            state['gen'] = Gen('plain')
        return state['gen']

    def run(bt):
        y = gen().run(*pwg_inputs('plain', *bt))
        return (y,), gen().path()

    def captured(bt):
        z, c, _ = pwg_inputs('plain', *bt)
        dz, dc = _dev(z, c)
        out = torch.zeros(bt[0], 1, bt[1] * 256, device='cuda')
        return lambda: gen().run_dev(dz, dc, None, out=out)

    try:
        _walk('pwg', [(1, 1), (1, 33), (1, 2), (8, 9)], run, release, lambda: gen().poison(), captured)
    finally:
        release()


def test_diffnet_prepare_under_capture():
    """The bound groups of the denoiser (GROW_BOUND): a prepare of a larger (B, T) under capture is refused and, as every
    refused prepare, leaves nothing bound; the small binding again and then the larger one, eagerly on the same handle, give a fresh handle's eps."""
    from bisinger_amd.diffnet import DiffNet
    use_config()
    net = load_formula_weights(DiffNet(80), 0, synth.DIFFNET_GAIN, prefix='denoise_fn.').cuda()
    lib = _lib.load()

    def inputs(B, T):
        g = torch.Generator().manual_seed(1000 * B + T)
        return torch.randn(B, 1, 80, T, generator=g).cuda(), torch.full((B,), 99, dtype=torch.long).cuda(), torch.randn(B, 256, T, generator=g).cuda()

    def run(B, T):
        x, t, cond = inputs(B, T)
        net.prepare(cond)
        eps = net(x, t, cond).cpu()
        return (eps,), net.last_path()

    net.release()
    want = run(2, 150)
    net.release()
    small = run(1, 40)
    cond = inputs(2, 150)[2]
    _refused_under_capture(lambda: _lib.check(lib.bsg_diffnet_prepare(net._h, _lib.ptr(cond), 2, 150, _lib.stream_ptr()), 'bsg_diffnet_prepare'),
                           'diffnet')
    net._bound = None      # (a refused prepare leaves nothing bound: tests/test_gpu_rebind.py)
    _same(run(1, 40), small, 'the small binding again, behind the refused prepare')
    _same(run(2, 150), want, 'the larger binding, eagerly')
    assert net.take_health() == (0, 0)
    net.release()
