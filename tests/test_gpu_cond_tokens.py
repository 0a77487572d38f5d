"""GPU: the conditioner term bound per token (bsg_diffnet_prepare_tokens) against the per-frame binding of the same condition
(bsg_diffnet_prepare on cond[b][:, f] = cond_tok[b][tok[b][f]]), model config as shipped (L = 20, C = 256).

Which launch runs is decided by the shape and by switches that a process reads once: at B = 2, T = 150 the default is a part form, and the
16-row launch on 64-frame tiles — the one with a token form — needs BSG_H2_NCT=2.  So the small-shape checks run in ONE child process
under that switch (a second child under BSG_H2_NCT=1 for that fallback); the child computes both sides and the tests compare what it
saved.  The two-launch-group shape takes 64-frame tiles by itself and runs here.

Expected everywhere: bit-identical.  The expansion of the token table is a copy, and the projection of a column turned out not to
depend on where the column sits in the GEMM (test_expanded_term_is_the_per_frame_term), so no cross-form bound is used.

The tile-class row: the ABI takes any ids in [0, K), so the run of sixteen 1-frame tokens inside one column tile of 16 frames cycles
through ids 2..9 (a front's mel2ph is monotone and has only 12 tokens here)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bisinger_amd import _lib, synth
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

B_S, T_S, K_S = 2, 150, 13      # three 64-frame tiles per row: first, interior, a 22-frame last


def tile_class_tokens():
    """tok [2][150] for T_txt = 12.  Row 0: token 1 on frames 0..15; frames 16..31 sixteen 1-frame tokens (one column tile); token 9 on
    32..59; token 10 on 60..135 (straddles the seams at 64 and 128, longer than a whole tile); token 11 has no frame; token 12 on
    136..143; 144..149 padding.  Row 1: twelve tokens of 11-12 frames, 10 frames of padding."""
    r0 = [1] * 16 + [2 + (i % 8) for i in range(16)] + [9] * 28 + [10] * 76 + [12] * 8 + [0] * 6
    r1 = [min(f * 12 // 140 + 1, 12) for f in range(140)] + [0] * 10
    assert len(r0) == T_S and len(r1) == T_S and 11 not in r0
    return torch.tensor([r0, r1], dtype=torch.long)


_CHILD = r'''
import sys, ctypes, torch
sys.path.insert(0, sys.argv[1])
torch.set_grad_enabled(False)
import bench
from bisinger_amd import _lib, synth
d = torch.load(sys.argv[2])
mode = sys.argv[4]
model = bench.build_model(torch.device('cuda', 0))
net, lib = model.denoise_fn, _lib.load()
cond_tok, tok, x = d['cond_tok'].cuda(), d['tok'].cuda(), d['x'].cuda()
B, K, H = cond_tok.shape
T = tok.shape[1]
cond = torch.stack([cond_tok[b, tok[b]] for b in range(B)]).transpose(1, 2).contiguous()
out = {}

def quads():
    q = torch.empty(net.n_layers, B, 128, T, 4, device='cuda')
    _lib.check(lib.bsg_diffnet_debug_cond_quads(net._h, _lib.ptr(q), B, T, _lib.stream_ptr()), 'bsg_diffnet_debug_cond_quads')
    return q.cpu()

def fwd(t):
    """one evaluation on whatever is bound (DiffNet.forward would bind its cond argument)"""
    tt = torch.full((B,), t, device='cuda', dtype=torch.long)
    eps = torch.empty(B, 80, T, device='cuda')
    _lib.check(lib.bsg_diffnet_forward(net._h, _lib.ptr(x[:, 0].contiguous()), _lib.ptr(tt), _lib.ptr(eps), B, T, _lib.stream_ptr()),
               'bsg_diffnet_forward')
    return eps.cpu(), net.last_path()

if mode == 'nct1':
    net.prepare_tokens(cond_tok, tok)
    out['tok'] = fwd(99)
    net.prepare(cond)
    out['frame'] = fwd(99)
    out['health'] = net.take_health()
    torch.save(out, sys.argv[3])
    sys.exit(0)

# (a) the expanded term against the per-frame one; (b) one evaluation; (c) 5 sampler steps, then a plain binding again
net.prepare(cond)
out['quads_frame'] = quads()
out['eps_frame'] = {t: fwd(t) for t in (99, 0)}
net.prepare_tokens(cond_tok, tok)
out['eps_tok'] = {t: fwd(t) for t in (99, 0)}
out['quads_tok'] = quads()
xs = x.clone()
out['x_tok'] = (model.sample(cond, xs, seed=5, n_steps=5, cond_tok=cond_tok, tok=tok).cpu(), net.last_path())
xs = x.clone()
out['x_frame'] = (model.sample(cond, xs, seed=5, n_steps=5).cpu(), net.last_path())

# fallbacks behind a token binding: the handle demoted AFTER the binding (the table is expanded) and, for one, before it
for name, off, on in (('h2q', lambda: net.set_q_launch(False), lambda: net.set_q_launch(True)),
                      ('h2', lambda: net.set_split_fp16(False), lambda: net.set_split_fp16(True)),
                      ('split', lambda: _lib.check(lib.bsg_diffnet_set_split(net._h, 0), 'set_split'),
                       lambda: _lib.check(lib.bsg_diffnet_set_split(net._h, 1), 'set_split'))):
    net.prepare_tokens(cond_tok, tok)
    off()
    a = fwd(99)
    net.prepare(cond)
    b = fwd(99)
    net.prepare_tokens(cond_tok, tok)      # bound in the demoted state: the call expands the condition itself
    c = fwd(99)
    on()
    out['fb_' + name] = (a, b, c)
out['health'] = net.take_health()

# shards: rows 2..3 of a batch of 4 — the sampler on the shard's slice of the token rows and of tok (Philox rows 2..3 of 4), and the whole
# model with rows= (its front rounds a shard's rows differently at these tiny shapes, with or without tokens: only the launch is looked at)
g = torch.Generator().manual_seed(29)
ct4 = torch.cat([cond_tok, torch.randn(2, K, H, generator=g).cuda()])
ct4[:, 0] = 0
tok4 = torch.cat([tok, tok.flip(0)])
x4 = torch.randn(4, 1, 80, T, generator=g).cuda()
cond4 = torch.stack([ct4[b, tok4[b]] for b in range(4)]).transpose(1, 2).contiguous()
full = model.sample(cond4, x4.clone(), seed=9, n_steps=3, cond_tok=ct4, tok=tok4).cpu()
p_full = net.last_path()
part = model.sample(cond4[2:4].contiguous(), x4[2:4].clone(), seed=9, n_steps=3, row0=2, B_total=4, cond_tok=ct4[2:4], tok=tok4[2:4]).cpu()
out['shard'] = (full, part, p_full, net.last_path())
inp = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_inputs(4, 12, T, seed=3, ragged=True).items()}
kw = {k: inp[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
k_step = model.K_step
model.K_step = 3
mel = model(inp['txt_tokens'], mel2ph=inp['mel2ph'], spk_embed=inp['spk_embed'], ref_mels=None, infer=True, seed=9, rows=slice(2, 4), **kw)['mel_out']
out['shard_model'] = (bool(torch.isfinite(mel).all()), tuple(mel.shape), net.last_path())
model.K_step = k_step
torch.save(out, sys.argv[3])
'''


def _inputs():
    g = torch.Generator().manual_seed(17)
    cond_tok = torch.randn(B_S, K_S, 256, generator=g)
    cond_tok[:, 0] = 0
    return {'cond_tok': cond_tok, 'tok': tile_class_tokens(), 'x': torch.randn(B_S, 1, 80, T_S, generator=g)}


def _child(tmp, nct, mode):
    src, dst = tmp / f'in_{mode}.pt', tmp / f'out_{mode}.pt'
    torch.save(_inputs(), src)
    env = dict(os.environ, BSG_H2_NCT=nct)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(src), str(dst), mode], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(dst)


@pytest.fixture(scope='module')
def small(tmp_path_factory):
    return _child(tmp_path_factory.mktemp('cond_tok'), '2', 'main')


@pytest.fixture(scope='module')
def model():
    import bench
    return bench.build_model(torch.device('cuda', 0))


def test_expanded_term_is_the_per_frame_term(small):
    """(a) the table expanded through tok equals what prepare(cond) writes: the projection of a column does not depend on its place in
    the GEMM (N = 26 token columns against 300 frames, other tile sizes)."""
    assert torch.equal(small['quads_tok'], small['quads_frame'])


def test_one_evaluation_equals_the_per_frame_launch(small):
    """(b) eps at t = 99 and t = 0: the token form against the per-frame 16-row launch on 64-frame tiles."""
    for t in (99, 0):
        eps_t, path_t = small['eps_tok'][t]
        eps_f, path_f = small['eps_frame'][t]
        assert (path_t, path_f) == ('stack_h2q_tok', 'stack_h2q')
        assert torch.isfinite(eps_t).all() and torch.equal(eps_t, eps_f), t


def test_five_sampler_steps_equal_the_per_frame_run(small):
    """(c) x after 5 steps (fused tail, Philox); the plain sample() behind it is back on the per-frame launch."""
    x_t, path_t = small['x_tok']
    x_f, path_f = small['x_frame']
    assert (path_t, path_f) == ('stack_h2q_tok_tail', 'stack_h2q_tail')
    assert torch.equal(x_t, x_f)
    assert small['health'] == (0, 0)


@pytest.mark.parametrize('name,paths', [('h2q', ('stack_h2',)), ('h2', ('split2', 'split4', 'wide', 'layer', 'stack_f43')),
                                        ('split', ('layer',))])
def test_fallbacks_behind_a_token_binding(small, name, paths):
    """bsg_diffnet_set_h2q / set_h2 / set_split(h, 0) behind (and in front of) a token binding: the launch that runs reads the expanded
    term and agrees with its own per-frame run bit for bit; no range event, no give-up."""
    (eps_a, path_a), (eps_b, path_b), (eps_c, path_c) = small['fb_' + name]
    assert path_a == path_b == path_c and path_a in paths, (path_a, path_b, path_c)
    assert torch.equal(eps_a, eps_b) and torch.equal(eps_c, eps_b)
    assert small['health'] == (0, 0)


def test_32_frame_tiles_behind_a_token_binding(tmp_path):
    """BSG_H2_NCT=1: the 16-row launch on 32-frame tiles has no token form and reads the expanded quads."""
    r = _child(tmp_path, '1', 'nct1')
    (eps_t, path_t), (eps_f, path_f) = r['tok'], r['frame']
    assert path_t == path_f == 'stack_h2q'
    assert torch.equal(eps_t, eps_f) and r['health'] == (0, 0)


def test_shard_rows_equal_the_unsharded_rows(small):
    """rows 2..3 of a batch of 4: the sampler on the shard's slice of the token rows and of tok equals the unsharded rows bit for bit, and
    the whole model with rows=slice(2, 4) (ragged T_txt, padded frames) binds the shard's token rows and takes the token form."""
    full, part, p_full, p_part = small['shard']
    assert p_full == p_part == 'stack_h2q_tok_tail'
    assert torch.equal(part, full[2:4])
    assert small['shard_model'] == (True, (2, T_S, 80), 'stack_h2q_tok_tail')


def test_two_launch_groups(model):
    """B = 3, T = 5650: 3 x 89 tiles of 64 frames > 256, two launch groups (the second starts at a row offset of the table and of tok)."""
    net = model.denoise_fn
    B, T, K = 3, 5650, 101
    g = torch.Generator().manual_seed(23)
    cond_tok = torch.randn(B, K, 256, generator=g).cuda()
    cond_tok[:, 0] = 0
    tok = (torch.arange(T) * (K - 1) // T + 1)[None].repeat(B, 1)
    tok[1, 5000:] = 0
    tok = tok.cuda()
    cond = torch.stack([cond_tok[b, tok[b]] for b in range(B)]).transpose(1, 2).contiguous()
    x = torch.randn(B, 1, 80, T, generator=g).cuda()
    got = model.sample(cond, x.clone(), seed=2, n_steps=2, cond_tok=cond_tok, tok=tok)
    assert net.last_path() == 'stack_h2q_tok_tail' and net.last_launch()[1] == 2
    want = model.sample(cond, x.clone(), seed=2, n_steps=2)
    assert net.last_path() == 'stack_h2q_tail' and net.last_launch()[1] == 2
    assert torch.equal(got, want)


def test_front_token_rows_are_the_frames_condition(model):
    """cond_tok[mel2ph] == decoder_inp bit for bit, B = 3 with ragged T_txt (padded tokens, padded frames)."""
    inp = {k: torch.from_numpy(v).cuda() for k, v in synth.synth_inputs(3, 12, 150, seed=5, ragged=True).items()}
    kw = {k: inp[k] for k in ('pitch_midi', 'midi_dur', 'is_slur', 'lang', 'speechsing')}
    ret = model.fs2(inp['txt_tokens'], inp['mel2ph'], inp['spk_embed'], None, None, None, None, skip_decoder=True, infer=True, **kw)
    ct, m2p, dec = ret['cond_tok'], ret['mel2ph'], ret['decoder_inp']
    assert tuple(ct.shape) == (3, 13, 256) and bool((m2p == 0).any()) and bool((ct[:, 0] == 0).all())
    got = torch.stack([ct[b, m2p[b]] for b in range(3)])
    assert torch.equal(got, dec)


def test_misuse(model):
    """K too small for tok: BSG_EINVAL and nothing bound; a null pointer: BSG_EINVAL."""
    net, lib = model.denoise_fn, _lib.load()
    h = net.handle()
    B, T, K = 2, 64, 5
    cond_tok = torch.randn(B, K, 256).cuda()
    tok = torch.randint(0, K, (B, T)).cuda()
    st = _lib.stream_ptr()
    assert lib.bsg_diffnet_prepare_tokens(h, _lib.ptr(cond_tok), _lib.ptr(tok), B, K - 1, T, st) == -22      # BSG_EINVAL
    assert b'outside' in lib.bsg_last_error()
    x, t, eps = torch.randn(B, 80, T).cuda(), torch.zeros(B, dtype=torch.long).cuda(), torch.empty(B, 80, T).cuda()
    assert lib.bsg_diffnet_forward(h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(eps), B, T, st) == -1                  # BSG_ESTATE
    assert lib.bsg_diffnet_prepare_tokens(h, None, _lib.ptr(tok), B, K, T, st) == -22
    assert lib.bsg_diffnet_prepare_tokens(h, _lib.ptr(cond_tok), None, B, K, T, st) == -22
    assert lib.bsg_diffnet_prepare_tokens(h, _lib.ptr(cond_tok), _lib.ptr(tok), B, 0, T, st) == -22
    net._bound = None
    net.prepare_tokens(cond_tok, tok)
    assert lib.bsg_diffnet_forward(h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(eps), B, T, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(eps).all()
