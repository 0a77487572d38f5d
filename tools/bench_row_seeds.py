"""Row-keyed draws against the in-kernel draws: what GaussianDiffusion.sample(row_seeds=) — one bsg_philox_normal_rows launch in front of
every step, its [B][80][T] buffer written and read back by the step's tail — costs over sample(seed=), whose tails draw in registers.
  fp32  B = 16, T = 1000, 100 DDPM steps (the headline shape)
  bf16  B = 64, T = 1000 (diff_compute_dtype bf16)
Per configuration the arms run interleaved, --repeats rounds of [unkeyed, keyed, unkeyed']: each round times --steps passes of every arm
after --warmup passes, device-synchronised.  unkeyed against unkeyed' (the same call twice in a round) is the A/A spread the keyed arm's
cost is read against.  One JSON line per configuration.

--parent-lib PATH: the unkeyed arm once more on another build of the library (the parent commit's, ABI v21: that process drops the two
v22 symbols from the binding), alternating with this build in child processes of their own, --build-repeats times each: has the unkeyed arm
moved beyond its A/A spread?

    python tools/bench_row_seeds.py [--steps K] [--warmup W] [--repeats R] [--dtype {fp32,bf16,both}] [--parent-lib PATH [--build-repeats N]]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {'fp32': (16, 1000), 'bf16': (64, 1000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5, help='timed passes per arm and round')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5, help='interleaved rounds')
    ap.add_argument('--dtype', choices=('fp32', 'bf16', 'both'), default='both')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--build-repeats', type=int, default=2, help='with --parent-lib: processes per build')
    ap.add_argument('--unkeyed-only', action='store_true', help='(the child of --parent-lib) time the unkeyed arm alone, print its ms per pass')
    ap.add_argument('--old-abi', action='store_true', help='(the child on the parent build) bind the library without the v22 symbols')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    if args.parent_lib and not args.unkeyed_only:
        compare_builds(args)
    from bisinger_amd import _lib
    if args.old_abi:
        for name in ('bsg_philox_normal_rows', 'bsg_ddpm_sample_rows'):
            _lib._SIGS.pop(name)
        _lib.ABI_VERSION = 21
    import torch
    import bench
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    model = bench.build_model(dev)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for dtype in (('fp32', 'bf16') if args.dtype == 'both' else (args.dtype,)):
        B, T = SHAPES[dtype]
        model.denoise_fn.set_compute(dtype)
        g = torch.Generator().manual_seed(1)
        cond = torch.randn(B, 256, T, generator=g).to(dev)
        x0 = torch.randn(B, 1, 80, T, generator=g).to(dev)
        seeds = [1000 + b for b in range(B)]
        unkeyed = lambda: model.sample(cond, x0.clone(), seed=3)      # noqa: E731
        keyed = lambda: model.sample(cond, x0.clone(), row_seeds=seeds)      # noqa: E731
        arms = (('unkeyed', unkeyed),) if args.unkeyed_only else (('unkeyed', unkeyed), ('keyed', keyed), ('unkeyed_again', unkeyed))
        paths = {}
        for name, fn in arms:
            timed(fn, args.warmup)
            paths[name] = model.denoise_fn.last_path()
        ms = {name: [] for name, _ in arms}
        for _ in range(args.repeats):
            for name, fn in arms:
                ms[name].append(timed(fn, args.steps))
        out = {'dtype': dtype, 'B': B, 'T': T, 'ddpm_steps': model.K_step, 'passes_per_round': args.steps, 'rounds': args.repeats,
               'lib': _lib.LIB_PATH, 'paths': paths, 'ms_per_pass': ms, 'median_ms': {k: statistics.median(v) for k, v in ms.items()}}
        if not args.unkeyed_only:
            med = out['median_ms']
            out['aa_spread'] = max(abs(a / b - 1) for a, b in zip(ms['unkeyed'], ms['unkeyed_again']))
            out['keyed_over_unkeyed'] = med['keyed'] / (0.5 * (med['unkeyed'] + med['unkeyed_again'])) - 1
            out['fill_bytes_per_step'] = B * 80 * T * 4
        print(json.dumps(out), flush=True)


def compare_builds(args):
    """The unkeyed arm on this build and on --parent-lib, alternating, each in a process of its own (a process binds one library)."""
    for dtype in (('fp32', 'bf16') if args.dtype == 'both' else (args.dtype,)):
        ms = {'this': [], 'parent': []}
        for _ in range(args.build_repeats):
            for which in ('this', 'parent'):
                cmd = [sys.executable, os.path.abspath(__file__), '--unkeyed-only', '--dtype', dtype, '--steps', str(args.steps), '--warmup', str(args.warmup),
                       '--repeats', '3'] + (['--old-abi'] if which == 'parent' else [])
                env = dict(os.environ, **({'BSG_LIB': os.path.abspath(args.parent_lib)} if which == 'parent' else {}))
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(f'{which} build failed:\n{p.stderr[-2000:]}')
                ms[which].append(json.loads(p.stdout.strip().splitlines()[-1])['median_ms']['unkeyed'])
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({'dtype': dtype, 'unkeyed_ms_per_pass_by_build': ms, 'median_ms': med, 'this_over_parent': med['this'] / med['parent'] - 1,
                          'spread_within_a_build': max(max(v) / min(v) - 1 for v in ms.values())}), flush=True)


if __name__ == '__main__':
    main()
