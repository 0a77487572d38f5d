#!/usr/bin/env python3
"""Which launch form every shape takes: the denoiser's planner, written down.

For an fp32 and a bf16 handle, B x T of the grid below, five handle states (default, bsg_diffnet_set_parts / set_h2q / set_h2 /
set_split 0) and three bindings (dense, per token with K = 8, ragged with lengths alternating T and ceil(T / 2)): one bsg_diffnet_forward,
then bsg_diffnet_last_path, bsg_diffnet_last_launch, bsg_diffnet_uses_handoffs and bsg_diffnet_ragged_native.  In the default state also a
2-step bsg_ddpm_sample and a 2-step bsg_plms_sample, with path and launch after each.  Everything through the C ABI, without the Python
guard: a call the library refuses is recorded as its error code.

    python tools/stack_form_census.py [OUT.json]      # default: tests/data/stack_form_census.json

tests/test_gpu_form_census.py runs census() again and compares with the committed file: a change to which form a shape takes is an edit
to that file."""
import json
import os
import sys
from ctypes import byref, c_int32

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, 'tests', 'data', 'stack_form_census.json')

DTYPES = ('fp32', 'bf16')
BATCHES = (1, 2, 3, 4, 5, 8, 9, 16, 17)
FRAMES = (32, 33, 64, 100, 1000)
STATES = ('default', 'set_parts', 'set_h2q', 'set_h2', 'set_split')      # but for 'default': bsg_diffnet_<state>(h, 0)
BINDINGS = ('dense', 'token', 'ragged')
K_TOK = 8
PLMS_T, PLMS_SPEEDUP = 10, 5      # bsg_plms_sample over t = 5, 0: two iterations


def ragged_lengths(B, T):
    return [T if b % 2 == 0 else (T + 1) // 2 for b in range(B)]


def census(device=0):
    """-> {"<dtype> <state> <binding> B=<B> T=<T>": record}; a record holds 'bind' (error code) alone where the binding is refused, else
    'forward' and, in the default state, 'ddpm' and 'plms': each [path, chains, groups] or an error code; and the two queries."""
    import bench
    from bisinger_amd import _lib
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', device)
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    Bm, Tm = max(BATCHES), max(FRAMES)
    cond_all = (0.5 * torch.randn(Bm, 256, Tm, generator=g)).to(dev)
    x_all = torch.randn(Bm, 80, Tm, generator=g).to(dev)
    ctok_all = (0.5 * torch.randn(Bm, K_TOK, 256, generator=g)).to(dev)
    ctok_all[:, 0] = 0
    out = {}
    with torch.cuda.device(dev):
        for dtype in DTYPES:
            model = bench.build_model(dev)
            net = model.denoise_fn
            net.set_compute(dtype)
            h = net.handle()
            sched, _keep = model._schedule()
            st = _lib.stream_ptr

            def launched(rc):
                if rc != 0:
                    return rc
                chains, groups = net.last_launch()
                return [net.last_path(), chains, groups]

            def query(fn, B, T):
                v = c_int32()
                rc = getattr(lib, fn)(h, B, T, byref(v))
                return v.value if rc == 0 else {'error': rc}

            for state in STATES:
                if state != 'default':
                    _lib.check(getattr(lib, 'bsg_diffnet_' + state)(h, 0), state)
                for binding in BINDINGS:
                    for B in BATCHES:
                        for T in FRAMES:
                            rec = out[f'{dtype} {state} {binding} B={B} T={T}'] = {}
                            cond = cond_all[:B, :, :T].contiguous()
                            if binding == 'dense':
                                rc = lib.bsg_diffnet_prepare(h, _lib.ptr(cond), B, T, st())
                            elif binding == 'token':
                                tok = (torch.arange(T, device=dev) * K_TOK // T).repeat(B, 1).contiguous()
                                rc = lib.bsg_diffnet_prepare_tokens(h, _lib.ptr(ctok_all[:B].contiguous()), _lib.ptr(tok), B, K_TOK, T, st())
                            else:
                                rc = lib.bsg_diffnet_prepare_ragged(h, _lib.ptr(cond), (c_int32 * B)(*ragged_lengths(B, T)), B, T, st())
                            if rc != 0:
                                rec['bind'] = rc
                                continue
                            x = x_all[:B, :, :T].contiguous()
                            t = torch.full((B,), 50, device=dev, dtype=torch.long)
                            eps = torch.empty_like(x)
                            rec['forward'] = launched(lib.bsg_diffnet_forward(h, _lib.ptr(x), _lib.ptr(t), _lib.ptr(eps), B, T, st()))
                            if state == 'default':
                                xs = x.clone()
                                rec['ddpm'] = launched(lib.bsg_ddpm_sample(h, byref(sched), _lib.ptr(xs), None, 7, 99, 2, B, T, 0, B, st()))
                                xs = x.clone()
                                rec['plms'] = launched(lib.bsg_plms_sample(h, byref(sched), _lib.ptr(xs), PLMS_T, PLMS_SPEEDUP, B, T, st()))
                            rec['uses_handoffs'] = query('bsg_diffnet_uses_handoffs', B, T)
                            rec['ragged_native'] = query('bsg_diffnet_ragged_native', B, T)
                    torch.cuda.synchronize()
                if state != 'default':
                    _lib.check(getattr(lib, 'bsg_diffnet_' + state)(h, 1), state)
            net.take_health()      # (no guard ran: leave no counted event behind on the device's words)
            net.release()
    return out


if __name__ == '__main__':
    path = sys.argv[1] if len(sys.argv) > 1 else DATA
    result = census()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(result, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{len(result)} cases -> {path}')
