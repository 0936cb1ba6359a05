"""CaptionTrainer.xe_step (frozen InceptionV3 at 224, COMIC-256, batch B) timed for the CNN plans bf16, f16 and bf16x3 in ONE
process on one GPU: images/s per plan as one JSON line.  B (default 64), STEPS (default 30), WARMUP (default 5)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from comic_amd import decoder as cdec, nets, trainer  # noqa: E402

B, STEPS, WARMUP = int(os.environ.get('B', '64')), int(os.environ.get('STEPS', '30')), int(os.environ.get('WARMUP', '5'))
rng = np.random.default_rng(0)
params = nets.CnnPlan('inception_v3', (224, 224)).init_params(0)
imgs = torch.from_numpy(rng.uniform(-1, 1, (B, 224, 224, 3)).astype(np.float32)).to('cuda:0')
caps = np.full((B, 16), -1, np.int64)
for b in range(B):
    n = 8 + b % 7
    caps[b, 0], caps[b, 1:n], caps[b, n] = 256, rng.integers(0, 256, n - 1), 257
out = {}
for dtype in ('bf16', 'f16', 'bf16x3'):
    x3 = dtype == 'bf16x3'
    plan = nets.CnnPlan('inception_v3', (224, 224), pool_after_projection=True, fuse_pools=not x3, x3=x3)
    tr = trainer.CaptionTrainer(params, cdec.DecoderSpec(), None, B, (224, 224), dtype, 'cuda:0', seed=8, plan=plan)
    tr.encoder.autotune()
    for _ in range(WARMUP):
        tr.xe_step(imgs, caps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        tr.xe_step(imgs, caps)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    out[dtype] = {'images_per_sec': round(B / dt, 1), 'ms_per_step': round(dt * 1e3, 3)}
    del tr
    torch.cuda.empty_cache()
out['f16_over_bf16'] = round(out['f16']['images_per_sec'] / out['bf16']['images_per_sec'], 4)
out['f16_over_bf16x3'] = round(out['f16']['images_per_sec'] / out['bf16x3']['images_per_sec'], 4)
out['config'] = 'CaptionTrainer.xe_step, InceptionV3 frozen 224, COMIC-256, batch %d, %d steps after %d warm-up' % (B, STEPS, WARMUP)
print(json.dumps(out))
