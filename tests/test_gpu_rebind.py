"""GPU: ONE denoiser handle walked through a sequence of bindings — shapes that shrink and grow, frames / tokens / ragged, both compute
modes, layouts derived on demand — against a FRESH handle per step, model config as shipped (L = 20, C = 256), default switches.

What this is after is the handle's buffer management between bindings: a capacity that no longer matches its buffers, a flag array
that is not zeroed after it was regrown, a layout marked as holding the bound term across a rebind.  Every such fault shows as a
difference between the walked handle and a handle that has seen nothing but the step's own binding, so the expectation everywhere is
bit-identical eps (t = 99 and t = 0), the same launch, and no range event or give-up.

STEPS is the one table both runs execute: the walk on one handle from top to bottom, the fresh runs one handle per row."""
import os
import subprocess
import sys

import pytest
import torch

from tests.test_gpu_cond_tokens import tile_class_tokens
from tests.util import ROOT

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# an action: ('frames', B, T) | ('tokens', B, T, K) | ('ragged', B, T, lens): bind (inputs are a function of the action alone);
# ('compute', dtype) | ('q', on) | ('h2', on): the handle's toggles; ('eval',): eps at t = 99 and t = 0 on what is bound, and the path
STEPS = [
    ('frames_2x150', [('frames', 2, 150), ('eval',)]),                       # first use: the part form's buffers
    ('frames_1x40', [('frames', 1, 40), ('eval',)]),                         # everything shrinks below capacity
    ('tokens_k13', [('tokens', 2, 150, 13), ('eval',)]),
    ('tokens_k29', [('tokens', 2, 150, 29), ('eval',)]),                     # the table and the planes grow by K alone
    ('frames_5x100', [('frames', 5, 100), ('eval',)]),                       # frames, flags and split scratch grow; a channel-split shape
    ('frames_16x64', [('frames', 16, 64), ('eval',)]),                       # the flag need grows again
    ('ragged_3x200', [('ragged', 3, 200, (200, 70, 129)), ('eval',)]),
    ('bf16_2x150', [('compute', 'bf16'), ('frames', 2, 150), ('eval',)]),
    ('bf16_4x130', [('compute', 'bf16'), ('frames', 4, 130), ('eval',)]),    # the bf16 group grows
    ('fp32_again', [('compute', 'fp32'), ('frames', 2, 150), ('eval',)]),
    # the 16-row launch switched off behind the binding, then on again and a rebind.  (On the default switches (2, 150) takes a part form
    # either way, which reads the quads: the rows are NOT derived here — 'rows_derived' below does that)
    ('q_launch_off_and_on', [('frames', 2, 150), ('q', False), ('eval',), ('q', True), ('frames', 2, 150), ('eval',)]),
    ('tokens_expanded', [('h2', False), ('tokens', 2, 150, 13), ('eval',), ('h2', True)]),   # the expanded-condition path
    # a handle demoted off the 16-bit pipe BEHIND the binding takes a channel-split launch, which reads rows: derived from the quads, with
    # condterm allocated on demand
    ('rows_derived', [('frames', 2, 150), ('h2', False), ('eval',), ('h2', True)]),
]
FAILED_LIKE = 'tokens_k13'     # the good prepare behind the failed one binds this step's tokens

_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
torch.set_grad_enabled(False)
import bench
from bisinger_amd import _lib
from tests.test_gpu_rebind import STEPS, FAILED_LIKE, tile_class_tokens
model = bench.build_model(torch.device('cuda', 0))
net, lib = model.denoise_fn, _lib.load()

def inputs(act):
    """the tensors of a binding: a function of the action alone, so the walk and the fresh runs bind the same values"""
    kind, B, T = act[:3]
    g = torch.Generator().manual_seed(1000 * B + T + (act[3] if kind == 'tokens' else 0))
    d = {'x': torch.randn(B, 80, T, generator=g).cuda()}
    if kind == 'tokens':
        K = act[3]
        d['cond_tok'] = torch.randn(B, K, 256, generator=g)
        d['cond_tok'][:, 0] = 0
        d['cond_tok'] = d['cond_tok'].cuda()
        if K == 13:
            d['tok'] = tile_class_tokens().cuda()
        else:       # K - 1 tokens of equal length; row 1 ends in 17 frames of padding
            tok = (torch.arange(T) * (K - 1) // T + 1)[None].repeat(B, 1)
            tok[1, T - 17:] = 0
            d['tok'] = tok.cuda()
    else:
        d['cond'] = torch.randn(B, 256, T, generator=g).cuda()
    return d

def fwd(x, t):
    """one evaluation on whatever is bound (DiffNet.forward would bind its cond argument)"""
    B, _, T = x.shape
    tt = torch.full((B,), t, device='cuda', dtype=torch.long)
    eps = torch.empty(B, 80, T, device='cuda')
    _lib.check(lib.bsg_diffnet_forward(net._h, _lib.ptr(x), _lib.ptr(tt), _lib.ptr(eps), B, T, _lib.stream_ptr()), 'bsg_diffnet_forward')
    return eps.cpu(), net.last_path()

def run(actions):
    rec, x = [], None
    for act in actions:
        if act[0] == 'compute': net.set_compute(act[1])
        elif act[0] == 'q': net.set_q_launch(act[1])
        elif act[0] == 'h2': net.set_split_fp16(act[1])
        elif act[0] == 'eval': rec.append([fwd(x, t) for t in (99, 0)])
        else:
            d = inputs(act)
            x = d['x']
            if act[0] == 'tokens': net.prepare_tokens(d['cond_tok'], d['tok'])
            elif act[0] == 'ragged':
                net.prepare(d['cond'], lengths=list(act[3]))
                assert net.ragged_native(act[1], act[2]), 'precondition: the ragged launch decodes this batch'
            else: net.prepare(d['cond'])
    return rec

out = {'walk': {}, 'fresh': {}}
for name, actions in STEPS:
    out['walk'][name] = run(actions)

# a failed prepare on the walked handle (K - 1 for ids up to K - 1), then a good one behind it
act = dict(STEPS)[FAILED_LIKE][0]
d = inputs(act)
B, T, K = act[1:]
st = _lib.stream_ptr()
eps = torch.empty(B, 80, T, device='cuda')
tt = torch.zeros(B, dtype=torch.long, device='cuda')
rc_prep = lib.bsg_diffnet_prepare_tokens(net._h, _lib.ptr(d['cond_tok']), _lib.ptr(d['tok']), B, K - 1, T, st)
err_prep = lib.bsg_last_error()
rc_fwd = lib.bsg_diffnet_forward(net._h, _lib.ptr(d['x']), _lib.ptr(tt), _lib.ptr(eps), B, T, st)
out['failed'] = (rc_prep, err_prep, rc_fwd, lib.bsg_last_error())
net._bound = None
out['after_failed'] = run(dict(STEPS)[FAILED_LIKE])
out['health_walk'] = net.take_health()

for name, actions in STEPS:
    net.set_compute('fp32')
    net.release()
    out['fresh'][name] = run(actions)
out['health_fresh'] = net.take_health()
torch.save(out, sys.argv[2])
'''


def run_child(dst, env=None):
    """the walk and the fresh runs in one child process on the default switches; returns what it saved"""
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, str(dst)], env=env or dict(os.environ), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(dst)


@pytest.fixture(scope='module')
def rebind(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp('rebind') / 'out.pt')


def _same(got, want):
    assert len(got) == len(want) and len(got) > 0
    for evals_g, evals_w in zip(got, want):
        for (eps_g, path_g), (eps_w, path_w) in zip(evals_g, evals_w):
            assert path_g == path_w, (path_g, path_w)
            assert torch.isfinite(eps_g).all() and torch.equal(eps_g, eps_w)     # (ragged: whole arrays, the padding's eps is 0)


@pytest.mark.parametrize('name', [s[0] for s in STEPS])
def test_walked_handle_equals_a_fresh_handle(rebind, name):
    """every evaluation of the step on the walked handle: eps bit-equal to, and the launch the same as, a fresh handle's."""
    _same(rebind['walk'][name], rebind['fresh'][name])


def test_no_range_event_no_give_up(rebind):
    assert rebind['health_walk'] == (0, 0) and rebind['health_fresh'] == (0, 0)


def test_failed_prepare_binds_nothing_and_a_good_one_follows(rebind):
    """a token prepare with K - 1: BSG_EINVAL and the forward is refused (BSG_ESTATE, nothing bound); the good prepare behind it on
    the same handle gives the fresh handle's result bit for bit."""
    rc_prep, err_prep, rc_fwd, err_fwd = rebind['failed']
    assert rc_prep == -22 and b'outside' in err_prep
    assert rc_fwd == -1 and b'does not match the condition bound' in err_fwd
    _same(rebind['after_failed'], rebind['fresh'][FAILED_LIKE])
