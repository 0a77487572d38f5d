"""Ragged batches against padding: real mel-frames/s of the diffusion decoder (GaussianDiffusion.sample, 100 DDPM steps, Philox noise) on
a ragged request list, three ways —
  padded    one batch padded to its longest row;
  bucketed  length buckets of max_sentences = 16 rows (bucket_by_size, as DiffSingerE2EInfer.forward_batch(max_sentences=16)), each padded
            to its own longest row, run one after another;
  ragged    one batch, every row at its own length (lengths=..., the ragged 16-row stack launch; --dtype bf16: the ragged bf16 stack
            launch and bf16 step tail).
Launch groups: the padded / bucketed batches run whole rows of ceil(T / 64) tiles, floor(CUs / tiles) rows per group; the ragged batch the
plan of bsg_ragged_plan.  Waste: padded frames computed for nothing.  Prints one JSON line per configuration:
  B = 64, lengths RandomState(0).randint(250, 1001)  (the request list of DESIGN section 4)
  B = 20 x T = 777                                  (uniform rows: 19 + 1 rows per group either way)

    python tools/bench_ragged.py [--steps K] [--warmup W] [--dtype {fp32,bf16}]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3, help='timed passes per mode')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--dtype', choices=('fp32', 'bf16'), default='fp32', help='the decoder configuration (bf16: diff_compute_dtype bf16)')
    args = ap.parse_args()
    sys.argv = sys.argv[:1]
    import numpy as np
    import torch
    import bench
    from bisinger_amd.diffnet import ragged_plan
    from bisinger_amd.infer import bucket_by_size
    torch.set_grad_enabled(False)
    dev = torch.device('cuda', 0)
    model = bench.build_model(dev)
    model.denoise_fn.set_compute(args.dtype)
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def groups_padded(B, T):
        return -(-B // (cus // -(-T // 64)))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    def run(name, lens):
        B, T = len(lens), max(lens)
        g = torch.Generator().manual_seed(1)
        cond = torch.randn(B, 256, T, generator=g).to(dev)
        x0 = torch.randn(B, 1, 80, T, generator=g).to(dev)
        real = int(sum(lens))
        buckets = bucket_by_size(lens, None, 16)
        parts = []
        for bk in buckets:
            Tb = max(lens[i] for i in bk)
            parts.append((cond[bk, :, :Tb].contiguous(), x0[bk, :, :, :Tb].contiguous(), Tb))
        modes = {}
        dt = timed(lambda: model.sample(cond, x0.clone(), seed=3))
        modes['padded'] = {'s_per_pass': dt, 'launch_groups': groups_padded(B, T), 'waste': 1 - real / (B * T), 'path': model.denoise_fn.last_path()}
        dt = timed(lambda: [model.sample(c, x.clone(), seed=3) for c, x, _ in parts])
        modes['bucketed16'] = {'s_per_pass': dt, 'launch_groups': sum(groups_padded(len(bk), Tb) for bk, (_, _, Tb) in zip(buckets, parts)),
                               'waste': 1 - real / sum(len(bk) * Tb for bk, (_, _, Tb) in zip(buckets, parts)), 'path': model.denoise_fn.last_path()}
        dt = timed(lambda: model.sample(cond, x0.clone(), seed=3, lengths=lens))
        modes['ragged'] = {'s_per_pass': dt, 'launch_groups': ragged_plan(lens, cus)[1], 'waste': 0.0, 'path': model.denoise_fn.last_path()}
        for m in modes.values():
            m['real_mel_frames_per_s'] = real / m['s_per_pass']
        r = modes['ragged']['real_mel_frames_per_s']
        print(json.dumps({'config': name, 'dtype': args.dtype, 'B': B, 'T_max': T, 'real_frames': real, 'tiles': int(sum(-(-n // 64) for n in lens)), 'cus': cus,
                          'ddpm_steps': model.K_step, 'modes': modes,
                          'ragged_speedup': {k: r / v['real_mel_frames_per_s'] for k, v in modes.items() if k != 'ragged'}}), flush=True)

    run('B64_U250_1000_seed0', [int(v) for v in np.random.RandomState(0).randint(250, 1001, size=64)])
    run('B20_T777', [777] * 20)


if __name__ == '__main__':
    main()
