"""What `--cnn_input_augment_crop area` / `--cnn_input_augment_color fast|full` cost, on ONE device in ONE process, at 64 JPEG
images of 640 x 480 -> 224 x 224 (synthetic photograph-like files, quality 90, 4:2:0):
  launches .. the preprocessing launches of the loader's entry alone (packed inverse DCT + the fused taps), device events
              around LAUNCHES calls, alternating rounds: `plain` (comic_jpeg_preprocess_packed), `plain_parent` (the same
              entry of another build of the library, PARENT_LIB=<libcomic_hip.so of the parent commit>, when given), `area`,
              `area_fast`, `area_full` (two passes) through comic_jpeg_preprocess_packed_aug
  loader .... images/s of the split-JPEG loader (JpegSplitPool on THREADS host threads, four batches in flight) for the same
              four settings, alternating rounds of REPS passes over 256 files
  host ...... the numpy colour distortion (augment.distort_color, `full`) of 224 x 224 images on 16 threads, per image
Medians with their ranges: one JSON line, printed and written to OUT (default profiles/r23_augment_time.json).
ROUNDS (default 7), LAUNCHES per round (default 500), WARMUP rounds (default 2), THREADS (default 16), REPS (default 40)."""
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from comic_amd import _lib as L, augment, inputs  # noqa: E402

ROUNDS, LAUNCHES, WARMUP, THREADS, REPS = (int(os.environ.get(k, d)) for k, d in (
    ('ROUNDS', '7'), ('LAUNCHES', '500'), ('WARMUP', '2'), ('THREADS', '16'), ('REPS', '40')))
OUT = os.environ.get('OUT', os.path.join(ROOT, 'profiles', 'r23_augment_time.json'))
PARENT_LIB = os.environ.get('PARENT_LIB', '')
DEV, N, OUT_H, OUT_W = 'cuda:0', 64, 224, 224


def make_files(count):
    from PIL import Image
    d = tempfile.mkdtemp()
    yy, xx = np.mgrid[0:480, 0:640]
    paths = []
    for i in range(count):
        rng = np.random.default_rng(i)
        base = np.stack([127 + 110 * np.sin(xx / (17.0 + i % 7) + i) * np.cos(yy / 13.0), 127 + 90 * np.cos((xx - yy) / (23.0 + i % 5)),
                         127 + 100 * np.sin((xx + 2 * yy) / 31.0 + i)], -1)
        img = np.clip(base + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8)
        p = os.path.join(d, '%d.jpg' % i)
        Image.fromarray(img).save(p, quality=90, subsampling=2)
        paths.append(p)
    return paths


paths = make_files(256)
lib = L.load()
SPECS = dict(area=augment.AugmentSpec('area', 'none'), area_fast=augment.AugmentSpec('area', 'fast'),
             area_full=augment.AugmentSpec('area', 'full'))

# ---- 1. the launches alone ----------------------------------------------------------------------------------------------------
jl = L.load_jpeg()
cap = sum(8 * os.path.getsize(p) + 64 for p in paths[:N])
infos, status, blob = np.zeros(N, L.JPEG_INFO_DTYPE), np.full(N, 99, np.int32), np.zeros(cap, np.uint16)
pool = jl.comic_jpeg_pool_create(THREADS)
h = jl.comic_jpeg_pool_submit_packed(pool, (C.c_char_p * N)(*[os.fsencode(p) for p in paths[:N]]), N, infos.ctypes.data,
                                     status.ctypes.data, blob.ctypes.data, cap)
used, planes_total = C.c_int64(-1), C.c_int64(-1)
assert h and jl.comic_jpeg_pool_wait(pool, h, 60.0, C.byref(used), C.byref(planes_total)) == 0 and (status == 0).all()
jl.comic_jpeg_pool_destroy(pool)
max_blocks = int(infos['coef_count'].max()) // 64
keys = inputs.draw_keys(N, __import__('random').Random(0)).keys
desc = np.zeros(N, inputs.DevicePreprocessor._DESC_DTYPE)
desc['in_h'], desc['in_w'] = infos['height'], infos['width']
desc['sy'], desc['sx'] = (infos['height'] / 256).astype(np.float32), (infos['width'] / 256).astype(np.float32)
plain = augment.augment_params(keys, infos['height'], infos['width'], augment.AugmentSpec('fixed', 'fast'))       # (its window)
desc['flip'], desc['oy'], desc['ox'] = plain.flip, plain.oy, plain.ox


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


d_blob, d_infos, d_desc = dev(blob[:used.value + (used.value & 1)]), dev(infos), dev(desc)
d_planes = torch.empty(planes_total.value + 4096, dtype=torch.uint8, device=DEV)
d_out = torch.empty((N, OUT_H, OUT_W, 3), dtype=torch.float32, device=DEV)
d_ws = torch.zeros(3 * N, dtype=torch.int64, device=DEV)
records = {}
for name, spec in SPECS.items():
    ap = augment.augment_params(keys, infos['height'], infos['width'], spec)
    dd = desc.copy()
    dd['flip'], dd['oy'], dd['ox'] = ap.flip, ap.oy, ap.ox
    records[name] = (dev(dd), dev(ap.aug), int(ap.contrast))


def plain_call(which):
    def fn():
        L.check(which.comic_jpeg_preprocess_packed(d_blob.data_ptr(), d_infos.data_ptr(), N, max_blocks, d_planes.data_ptr(), None,
                                                   d_desc.data_ptr(), d_out.data_ptr(), OUT_H, OUT_W, 256, L.stream_ptr()), 'plain')
    return fn


def aug_call(name):
    dd, da, contrast = records[name]

    def fn():
        L.check(lib.comic_jpeg_preprocess_packed_aug(d_blob.data_ptr(), d_infos.data_ptr(), N, max_blocks, d_planes.data_ptr(), None,
                                                     dd.data_ptr(), da.data_ptr(), contrast, d_ws.data_ptr(), d_out.data_ptr(),
                                                     OUT_H, OUT_W, 256, L.stream_ptr()), name)
    return fn


sides = dict(plain=plain_call(lib))
if PARENT_LIB:
    parent = C.CDLL(PARENT_LIB)
    parent.comic_jpeg_preprocess_packed.restype, parent.comic_jpeg_preprocess_packed.argtypes = L._SIGS['comic_jpeg_preprocess_packed']
    sides['plain_parent'] = plain_call(parent)
sides.update({name: aug_call(name) for name in SPECS})


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES * 1e3            # microseconds per call


for _ in range(WARMUP):
    for fn in sides.values():
        timed(fn)
launch = {k: [] for k in sides}
for _ in range(ROUNDS):
    for k, fn in sides.items():
        launch[k].append(timed(fn))
assert bool(torch.isfinite(d_out).all())


# ---- 2. the loader ------------------------------------------------------------------------------------------------------------
def loader_side(spec):
    jpool = inputs.JpegSplitPool(THREADS, max_batch=N)
    pre = inputs.DevicePreprocessor(DEV, OUT_H, OUT_W, spec=spec)
    pre.enable_split(jpool, 6)
    rng = __import__('random').Random(1)

    def one_round():
        n, t0, inflight = 0, time.time(), []
        for _ in range(REPS):
            for b in range(0, len(paths), N):
                ps = paths[b:b + N]
                params = (inputs.draw_keys(len(ps), rng) if spec is not None
                          else [inputs.draw_augmentation(True, OUT_H, OUT_W, rng) for _ in ps])
                inflight.append(pre.pack_paths_split(ps, params))
                if len(inflight) > 3:
                    pre.finish(inflight.pop(0))
                n += len(ps)
        while inflight:
            pre.finish(inflight.pop(0))
        torch.cuda.synchronize()
        return n / (time.time() - t0)
    return one_round, jpool


loaders = {k: loader_side(s) for k, s in [('plain', None)] + list(SPECS.items())}
for fn, _ in loaders.values():
    fn()
loader = {k: [] for k in loaders}
for _ in range(max(3, ROUNDS // 2)):
    for k, (fn, _) in loaders.items():
        loader[k].append(fn())
for _, jp in loaders.values():
    jp.close()

# ---- 3. the host colour distortion, for scale -------------------------------------------------------------------------------------
rng = np.random.default_rng(0)
imgs = [rng.random((OUT_H, OUT_W, 3), dtype=np.float32) for _ in range(64)]
recs = augment.augment_params(keys, [480] * N, [640] * N, SPECS['area_full']).aug
host = []
with ThreadPoolExecutor(max_workers=16) as tp:
    for _ in range(3):
        t0 = time.time()
        list(tp.map(lambda a: augment.distort_color(a[0], a[1]), zip(imgs, recs)))
        host.append((time.time() - t0) / len(imgs) * 1e3)

out = {}
for k, x in launch.items():
    out['launch_%s_us' % k] = round(statistics.median(x), 2)
    out['launch_%s_us_min_max' % k] = [round(min(x), 2), round(max(x), 2)]
for k, x in loader.items():
    out['loader_%s_images_per_s' % k] = round(statistics.median(x))
    out['loader_%s_images_per_s_min_max' % k] = [round(min(x)), round(max(x))]
out['host_distort_color_full_ms_per_image_16_threads'] = round(statistics.median(host), 3)
out['config'] = ('%d JPEG files of 640 x 480 (4:2:0, quality 90) -> %d x %d, area_min 0.35; launches: the packed entry on a resident '
                 'batch, median of %d alternating rounds of %d calls after %d warm-up rounds, device events; loader: split decode on '
                 '%d host threads, four batches in flight, %d passes over 256 files per round; host: numpy on 16 threads, '
                 'wall time per image' % (N, OUT_H, OUT_W, ROUNDS, LAUNCHES, WARMUP, THREADS, REPS))
line = json.dumps(out)
print(line)
with open(OUT, 'w') as f:
    f.write(line + '\n')
