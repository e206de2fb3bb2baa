#!/usr/bin/env python
"""Step time of a full-size training configuration with the training knobs on or off (csrc/loss.hip LS1-LS4, csrc/elementwise.hip GC1-GC3,
WD1): bench.py's timed protocol -- W warm-up steps, then K pipelined trainIterations on a fresh batch each -- through NativeModel, one JSON
line.  The kernel times of profiles/train_knobs.txt come from running this under `rocprofv3 --kernel-trace --stats`.

  python scripts/mb_train_knobs.py --config 3 --steps 30 --warmup 10                                  # knobs off: the bench.py headline
  python scripts/mb_train_knobs.py --config 3 --labelSmoothing 0.1 --gradClipNorm 10 --weightDecay 1e-4
  python scripts/mb_train_knobs.py --config 1 --labelSmoothing 0.1                                    # lf-ques-im-hist + gen"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, choices=[1, 3], default=3, help='bench.py config: 3 = mn-att-ques-im-hist + disc (headline), 1 = lf-ques-im-hist + gen')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--labelSmoothing', type=float, default=None)
    ap.add_argument('--gradClipNorm', type=float, default=None)
    ap.add_argument('--weightDecay', type=float, default=None)
    a = ap.parse_args()
    from bench import config_params
    from visdial_amd.dataloader import SyntheticDataloader
    from visdial_amd.native import NativeModel
    p = config_params(a.config, batch=a.batch)
    knobs = {k: getattr(a, k) for k in ('labelSmoothing', 'gradClipNorm', 'weightDecay')}
    p.update(knobs)
    model = NativeModel(p)
    dl = SyntheticDataloader(p, seed=1234, fast=True)
    for _ in range(a.warmup):
        model.trainIteration(dl)
    model.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = model.trainIteration(dl)
    model.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    n = sum(r * c for _, _, r, c in model.tensors)
    model.close()
    print(json.dumps(dict(config=a.config, knobs=knobs, steps=a.steps, warmup=a.warmup, ms_per_step=round(ms, 3), loss=round(float(loss), 5),
                          parameters=n, library=os.environ.get('VD_LIB_PATH', 'default'))))


if __name__ == '__main__':
    main()
