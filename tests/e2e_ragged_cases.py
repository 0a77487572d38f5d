"""Items, state dicts and the float64 "alone" chain of the end-to-end ragged tests: what tests/test_e2e_ragged_cpu.py (CPU) and
tests/test_gpu_e2e_ragged.py (GPU) share.  No GPU is needed to import this module.

The property under test: DiffSingerE2EInfer.forward_batch(items, ragged_front=True, ragged=True, ragged_pitch=True, ragged_vocoder=True,
denoise_c=...) gives every item what the pipeline gives for that utterance ALONE (B = 1 on its own tokens and frames), with the random
draws it meets in its bucket: the sampler's and the NSF source's Philox streams are indexed by the row's place b in a bucket of B rows at
the bucket's padded frame count T.

alone_chain() is that statement, written only from existing oracle functions (oracle.fs2.fs2_forward, oracle.melgen.mel_gen,
oracle.pe.pitch_extractor_forward, oracle.hifigan.hifigan_forward / oracle.nsf.nsf_hifigan_forward, tests.wavden_ref.denoise) plus the
slicing of the draws; it holds no arithmetic of its own (tests/test_e2e_ragged_cpu.py: in float32 at b = 0, B = 1, T = n it IS the padded
oracle composition of tests/test_gpu_infer.py on the lone item, bit for bit).

Items.  Five items of 3 to 8 tokens (SPECS: token count and the seed of item()), plain dicts of numpy arrays with the keys infer.collate
reads.  The formula weights round about half of the durations to 0, so the duration predictor's bias is raised by RAISE
(tests/dur_cases.RAISE, as tests/test_gpu_fs2_ragged._diffusion does) by raise_dur_bias(), the one helper for the state dict the chain reads
and for the checkpoint the GPU test loads.  The items were chosen on the CPU with the float64 chain so that (conditions(), evaluated again by
the CPU test):
  * the alone frame counts cover: one n < 64; one 64 < n < 128 with n % 4 != 0; one n > 128 with n % 4 != 0; one n % 64 == 0 (the
    denoiser's tile is 64 frames; a row with n % 4 != 0 takes other GEMM forms when it runs alone);
  * estimate_frames is distinct for all five, so a bucket's row order does not depend on the order the items are given in;
  * max_sentences = 3 gives two buckets whose order differs from the given order;
  * NO token's predicted duration is undecided (tests/dur_cases.undecided at fs2_ragged_cases.BOUND['dur']);
  * every row has at least one frame;
  * in the NSF set-up, the frames of the float64 chain whose voicing logit lies within the pitch extractor's bound of zero (10 bars of
    tests/test_gpu_f2_fullsize._check_pitch) stay under fs2_ragged_cases.TIE_CAP of every row.
"""
import hashlib
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from bisinger_amd import synth
from oracle import diffusion as odf, fs2 as ofs2, hifigan as ohg, melgen as omg, nsf as onsf, pe as ope
from tests import dur_cases as DC
from tests import fs2_ragged_cases as RC
from tests import wavden_ref

F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')

SEED = 77
MAX_SENTENCES = 3
DENOISE_C = 0.1
STEPS = 100                   # the schedule of the workdir fixture (bisinger_diff100.yaml)
HOP = 256                     # the vocoder's samples per frame (prod of hifigan.yaml's upsample_rates)
NH = 9                        # NSF harmonics + 1
NSF_STREAM = 0x4E5346         # the Philox stream of the NSF noise (bisinger_amd/hifigan.py)
TRIPLE = (512, 128, 512)      # fft_size, hop_size, win_size of the post-filter (bisinger_base.yaml)
RAISE = DC.RAISE              # added to fs2.dur_predictor.linear.bias
SETUPS = ('plain', 'nsf')     # the workdir fixture of tests/test_gpu_infer.py; the nsf_workdir fixture of tests/test_gpu_pe_ragged.py

# (tokens, seed of item()) in the order the items are GIVEN; the float64 alone frame counts are FRAMES (held by the CPU test)
# estimate_frames 168, 454, 292, 173, 546 -> buckets [4, 1, 2] (rows of 65, 135, 64 frames at T = 135) and [3, 0] (81, 29 at T = 81): the
# longest row of the first bucket is its middle one, 65 is one frame over the denoiser's tile, 64 fills it
SPECS = ((3, 3), (7, 5), (5, 10), (3, 2), (6, 6))
FRAMES = (29, 135, 64, 81, 65)
BUCKETS = ((4, 1, 2), (3, 0))

# Yardsticks: the largest deviation of the float32 alone_chain from the float64 one over the five items at their row places, measured on
# the CPU (tests/test_e2e_ragged_cpu.py::test_yardsticks evaluates them again and holds every figure to its entry); x max(1, max |want|), f0
# relative to max(1, f0) away from the voicing edge.  They are the float32 ORACLE's error, never the device's.  Float32 CPU kernels differ
# in their last bits with the thread count and the vector width (the vocoder's figures moved by up to 5 % between 4, 8 and 16 threads; the
# front's and the sampler's did not move), so each entry is the largest figure seen plus 3 %, rounded up in its second digit.
# HANDOFF: every float32 stage fed the float64 previous stage.  COMPOSED: no feed (NSF set-up: the float64 f0 fed, as the sine source
# integrates f0).  The GPU test's bars are 4 x these where a stage has no project bar of its own.  Largest figures seen:
#   hand-off  decoder_inp 2.637e-7  mel_out 6.803e-7  pitch_pred 3.305e-6  f0 3.201e-6  wav 1.044e-6 (plain) 1.459e-6 (nsf)
#             wav_denoised 1.937e-7 (plain) 3.140e-7 (nsf)
#   composed  mel_out 7.688e-7  wav 1.160e-6 (plain) 1.487e-6 (nsf)  wav_denoised 1.124e-6 (plain) 1.438e-6 (nsf)
YARD_HANDOFF = {'plain': {'decoder_inp': 2.8e-7, 'mel_out': 7.1e-7, 'wav': 1.1e-6, 'wav_denoised': 2.0e-7},
                'nsf': {'decoder_inp': 2.8e-7, 'mel_out': 7.1e-7, 'pitch_pred': 3.5e-6, 'f0': 3.3e-6, 'wav': 1.6e-6, 'wav_denoised': 3.3e-7}}
YARD_COMPOSED = {'plain': {'mel_out': 8.0e-7, 'wav': 1.2e-6, 'wav_denoised': 1.2e-6}, 'nsf': {'mel_out': 8.0e-7, 'wav': 1.6e-6, 'wav_denoised': 1.5e-6}}


# ------------------------------------------------------------------------------------------------------------------
# items
# ------------------------------------------------------------------------------------------------------------------
def item(nt, seed):
    """One item of nt tokens: what preprocess_input returns (the keys collate reads), without the phoneme front."""
    rs = np.random.RandomState(1000 * nt + seed)
    return {'item_name': f'e2e-{nt}-{seed}', 'text': 'x', 'ph': ' '.join(['<AP>'] * nt), 'spk_id': 3 if seed % 2 else 7,
            'ph_token': np.concatenate([[3], rs.randint(4, 64, size=nt - 1)]).astype(np.int64),
            'pitch_midi': rs.choice([60, 63, 54, 69, 0, 64], size=nt).astype(np.int64),
            'midi_dur': np.round(rs.uniform(0.1, 0.6, size=nt), 3), 'is_slur': rs.randint(2, size=nt).astype(np.int64),
            'lang': rs.randint(2, size=nt).astype(np.int64), 'speechsing': 1}


def items():
    return [item(nt, s) for nt, s in SPECS]


def lone_inputs(it):
    """The item as the B = 1 batch infer.collate makes of it, in the oracle's names (CPU tensors)."""
    t = lambda k, dt: torch.as_tensor(np.asarray(it[k]))[None].to(dt)      # noqa: E731
    return {'txt_tokens': t('ph_token', torch.long), 'spk_embed': torch.tensor([int(it['spk_id'])]), 'pitch_midi': t('pitch_midi', torch.long),
            'midi_dur': t('midi_dur', torch.float32), 'is_slur': t('is_slur', torch.long), 'lang': t('lang', torch.long),
            'speechsing': torch.tensor([int(it['speechsing'])])}


# ------------------------------------------------------------------------------------------------------------------
# state dicts: the recipes of the fixtures (tests/conftest.py gd_sd / hifigan_sd, tests/test_gpu_pe_ragged.py nsf_workdir)
# ------------------------------------------------------------------------------------------------------------------
def raise_dur_bias(sd, prefix=''):
    """fs2.dur_predictor.linear.bias + RAISE, in float32, in place on a state dict whose keys start with `prefix` ('model.' in a checkpoint)."""
    k = prefix + 'fs2.dur_predictor.linear.bias'
    sd[k] = (sd[k].float() + np.float32(RAISE)).float()
    return sd


def raise_checkpoint(path):
    """The same on a checkpoint file of the synthetic checkpoint directory."""
    ck = torch.load(path, map_location='cpu')
    raise_dur_bias(ck['state_dict'], 'model.')
    torch.save(ck, path)


_SDS = {}


def state_dicts(setup):
    """-> dict(model, voc, voc_cfg, pe (None in the plain set-up), nsf): CPU state dicts of the set-up, the duration bias raised."""
    if setup in _SDS:
        return _SDS[setup]
    import yaml
    with open(os.path.join(GOLD, 'state_dict_spec.json')) as f:
        js = json.load(f)
    od = lambda name: OrderedDict((k, tuple(s)) for k, s in js[name])      # noqa: E731
    if 'model' not in _SDS:
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(od('GaussianDiffusion'), 0, synth.DIFFNET_GAIN).items()}
        sd.update(odf.make_schedule(STEPS, 'linear', 0.06))
        g = np.load(os.path.join(GOLD, 'schedules.npz'))
        sd['spec_min'], sd['spec_max'] = torch.from_numpy(g['spec_min']), torch.from_numpy(g['spec_max'])
        _SDS['model'] = raise_dur_bias(sd)
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'bisinger_amd', 'configs', 'hifigan.yaml')))
    out = {'model': _SDS['model'], 'nsf': setup == 'nsf', 'pe': None}
    if setup == 'plain':
        out['voc'] = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(od('HifiGanGenerator_weight_norm'), 7).items()}
    else:
        cfg['use_pitch_embed'] = True
        out['voc'] = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(od('HifiGanGenerator_nsf_weight_norm'), seed=13).items()}
        spec = od('PitchExtractor')
        pw = synth.synth_state_dict(spec, seed=11)
        for k in spec:
            if k.endswith('running_var'):
                pw[k] = (0.5 + np.abs(pw[k]) * 5).astype(np.float32)
        pe = {k: torch.from_numpy(v) for k, v in pw.items()}
        for k, s_ in spec.items():
            if k not in pe:
                pe[k] = torch.zeros(s_, dtype=torch.long if k.endswith('num_batches_tracked') else torch.float32)
        out['pe'] = pe
    out['voc_cfg'] = cfg
    _SDS[setup] = out
    return out


# ------------------------------------------------------------------------------------------------------------------
# the device's own random streams (bisinger_amd/synth.py restates the library's Philox4x32-10)
# ------------------------------------------------------------------------------------------------------------------
_DRAWS = {}


def _stream(seed, stream, count):
    key = (seed, stream, count)
    if key not in _DRAWS:
        _DRAWS[key] = synth.philox_normal(seed, stream, count)
    return _DRAWS[key]


def sampler_noise(b, B, T, n, seed):
    """[STEPS + 1, 1, 80, n]: x_T (stream 0) and the draw of every executed step (stream i + 1 for step i, i = STEPS - 1 .. 0) of row b
    of a bucket of B rows at T frames: the layout of tests/test_gpu_infer._oracle_wav, sliced [b, :, :n]."""
    cnt = B * 80 * T
    z = np.stack([_stream(seed, 0, cnt)] + [_stream(seed, i + 1, cnt) for i in reversed(range(STEPS))])
    return torch.from_numpy(np.ascontiguousarray(z.reshape(STEPS + 1, B, 80, T)[:, b:b + 1, :, :n]))


def nsf_draws(b, B, T, n, seed):
    """(rand_ini [1, NH], noise [1, n HOP, NH]) of row b: HifiGanGenerator._forward draws RandomState(seed & 0x7FFFFFFF).uniform((B, NH)) and
    the Philox stream NSF_STREAM over (B, T HOP, NH) at the padded T of the call, ragged or not."""
    ri = np.random.RandomState(seed & 0x7FFFFFFF).uniform(size=(B, NH)).astype(np.float32)[b:b + 1]
    nz = _stream(seed, NSF_STREAM, B * T * HOP * NH).reshape(B, T * HOP, NH)[b:b + 1, :n * HOP]
    return torch.from_numpy(ri.copy()), torch.from_numpy(np.ascontiguousarray(nz))


# ------------------------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------------------------
_MEL = {}      # the sampler is the cost (100 evaluations of the denoiser): one result per distinct call, shared by both set-ups


def _digest(a):
    return None if a is None else hashlib.sha1(np.ascontiguousarray(np.asarray(a)).tobytes()).hexdigest()


def alone_chain(sds, it, b, B, T, seed, dtype, feed=None):
    """The item at B = 1 on its own tokens, every stage in `dtype`, with the draws of row b of a bucket of B rows at T frames.
    -> dict of numpy arrays: dur [nt] (the duration predictor's log-domain output), dur_choice [nt], mel2ph [n], n, decoder_inp [n, 256],
    mel_out [n, 80], with the NSF set-up pitch_pred [n, 2], f0 [n], uv [n]; wav [n HOP], wav_denoised [n HOP].

    feed (hand-off mode): dict of arrays that REPLACE a stage's input — 'decoder_inp' [n, 256] for the sampler, 'mel_out' [n, 80] for the
    pitch extractor and the vocoder, 'f0' [n] for the NSF source, 'wav' [n HOP] for the post-filter.  Every stage without a fed input takes
    the chain's own previous output."""
    feed = feed or {}
    npd = np.float64 if dtype == F64 else np.float32
    inp = lone_inputs(it)
    sd = sds['model']
    mkey = (it['item_name'], b, B, T, seed, str(dtype), _digest(feed.get('decoder_inp')))
    if mkey not in _MEL:
        f = ofs2.fs2_forward(sd, inp, dtype=dtype)
        n = int(f['mel2ph'].shape[1])
        assert n <= T, (it['item_name'], n, T)
        front = {'dur': f['dur'][0, :, 0], 'dur_choice': f['dur_choice'][0], 'mel2ph': f['mel2ph'][0], 'decoder_inp': f['decoder_inp'][0]}
        if 'decoder_inp' in feed:
            f = dict(f, decoder_inp=torch.as_tensor(np.asarray(feed['decoder_inp'])).to(dtype)[None])
        r = omg.mel_gen(sd, inp, sampler_noise(b, B, T, n, seed), fs2_out=f, dtype=dtype)
        _MEL[mkey] = dict(front, n=n, mel_out=r['mel_out'][0])
    out = dict(_MEL[mkey])
    n = out['n']
    mel = torch.as_tensor(np.asarray(feed['mel_out'])).to(dtype) if 'mel_out' in feed else out['mel_out']
    f0 = None
    if sds['pe'] is not None:
        p = ope.pitch_extractor_forward(sds['pe'], mel[None], dtype=dtype)
        out.update(pitch_pred=p['pitch_pred'][0], f0=p['f0_denorm_pred'][0], uv=p['pitch_pred'][0, :, 1] > 0)
        f0 = torch.as_tensor(np.asarray(feed['f0'])).to(dtype) if 'f0' in feed else out['f0']
    if sds['nsf']:
        assert f0 is not None
        ri, nz = nsf_draws(b, B, T, n, seed)
        wav = onsf.nsf_hifigan_forward(sds['voc'], mel.transpose(0, 1)[None], f0[None], ri, nz, sds['voc_cfg'], dtype=dtype)[0, 0]
    else:
        wav = ohg.hifigan_forward(sds['voc'], mel.transpose(0, 1)[None], sds['voc_cfg'], dtype=dtype)[0, 0]
    out['wav'] = wav
    out = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    src = np.asarray(feed['wav']) if 'wav' in feed else out['wav']
    out['wav_denoised'] = wavden_ref.denoise(src, DENOISE_C, *TRIPLE, dtype=npd)
    return out


# ------------------------------------------------------------------------------------------------------------------
# buckets and the conditions on the items
# ------------------------------------------------------------------------------------------------------------------
def buckets(its):
    """(estimated frames, buckets of indices) as forward_batch(max_sentences=MAX_SENTENCES) forms them (its own functions)."""
    from bisinger_amd.infer import DiffSingerE2EInfer, bucket_by_size
    from tests.util import use_config
    use_config()
    est = [DiffSingerE2EInfer.estimate_frames(None, it) for it in its]
    return est, bucket_by_size(est, None, MAX_SENTENCES)


def places(its, frames):
    """index -> (b, B, T): every item's row place in its bucket, the bucket's rows and its padded frame count."""
    out = {}
    for bk in buckets(its)[1]:
        T = max(frames[i] for i in bk)
        for b, i in enumerate(bk):
            out[i] = (b, len(bk), T)
    return out


def front_only(it, dtype=F64):
    """(n, dur xs [nt] float64 numpy) of the lone item: the front without its decoder."""
    f = ofs2.fs2_forward(state_dicts('plain')['model'], lone_inputs(it), dtype=dtype, skip_decoder=True)
    return int(f['mel2ph'].shape[1]), f['dur'][0, :, 0].double().numpy()


def uv_margin(pitch_pred64, pitch_pred32):
    """The pitch extractor's bar (tests/test_gpu_f2_fullsize._check_pitch: 2 x the float32 oracle's deviation + 2e-5 of the scale) and the
    frames whose voicing logit lies within 10 bars of zero: they may fall either way."""
    pp64 = np.asarray(pitch_pred64, np.float64)
    dev32 = float(np.abs(np.asarray(pitch_pred32, np.float64) - pp64).max())
    bar = 2 * dev32 + 2e-5 * max(1.0, float(np.abs(pp64).max()))
    return bar, np.abs(pp64[..., 1]) <= 10 * bar


def conditions(its, frames, xs):
    """The conditions of the module docstring that need the front only -> list of (item name or 'items', condition) that FAIL.
    frames[i], xs[i]: front_only(its[i])."""
    bad = []
    names = [it['item_name'] for it in its]
    if len(its) != 5 or not all(3 <= len(it['ph_token']) <= 8 for it in its):
        bad.append(('items', 'five items of 3 to 8 tokens'))
    for cond, what in ((lambda n: n < 64, 'one n < 64'), (lambda n: 64 < n < 128 and n % 4, 'one 64 < n < 128 with n % 4 != 0'),
                       (lambda n: n > 128 and n % 4, 'one n > 128 with n % 4 != 0'), (lambda n: n % 64 == 0, 'one n % 64 == 0')):
        if not any(cond(n) for n in frames):
            bad.append(('items', f'no frame count of the class: {what} (frames {list(frames)})'))
    est, bks = buckets(its)
    if len(set(est)) != len(est):
        bad.append(('items', f'estimate_frames not distinct: {est}'))
    if len(bks) != 2 or [i for bk in bks for i in bk] == list(range(len(its))):
        bad.append(('items', f'max_sentences={MAX_SENTENCES} does not give two buckets in another order than given: {bks}'))
    for name, it, n, x in zip(names, its, frames, xs):
        if n < 1:
            bad.append((name, 'no frame'))
        loose = DC.undecided(x[None], np.ones((1, len(x)), bool), RC.BOUND['dur'])
        if loose.any():
            bad.append((name, f'undecided duration at token(s) {np.nonzero(loose[0])[0].tolist()}'))
    return bad


def norm_dev(got, want):
    """max |got - want| / max(1, max |want|): the project's normalisation."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def f0_dev(got, want, skip=None):
    """max |got - want| / max(1, want) over the frames not in `skip`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    keep = np.ones(want.shape, bool) if skip is None else ~np.asarray(skip)
    return float((np.abs(got - want) / np.maximum(want, 1.0))[keep].max()) if keep.any() else 0.0
