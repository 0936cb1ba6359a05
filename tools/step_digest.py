"""Bit digests of the teacher-forced decoder executor (comic_decoder_train_step / comic_decoder_score) over the branches of
csrc/decoder_exec.hip, through the Python Decoder API only -- the same file runs against any build of the library
(COMIC_HIP_LIB=<other libcomic_hip.so>), and two builds that issue the same device operations print the same lines.
   python tools/step_digest.py [--fields]
Per case, for fixed seeds, one train_step(want_input_grads=True) with every dropout on (device-generated masks of a fixed
seed) and SCST rewards, and one score() of the same captions; one sha256 over loss, map loss, logits, ids, attention maps, the
flat gradient, dfm, dim_embed, token and caption log-probabilities and the reported train / score path.  Cases: the
geometries of tests/test_gpu_path.py's TRAIN_VARIANTS at B = 6, the COMIC-256 geometry at B = 23 and 64 (both persistent
loops), and that geometry under each executor switch that selects another branch (the environment switches of
comic_amd/_lib.py, and the two-call fwd / bwd phase form)."""
import ast
import hashlib
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from comic_amd import decoder as cdec  # noqa: E402

DEV = 'cuda:0'
BASE = dict(D=128, E=64, V=258, C=192, Cg=192, H=8, M=25)          # tests/test_gpu_path.py: _spec_and_cfg
COMIC256 = dict(D=512, E=256, C=2048, Cg=2048)
SWITCHES = [                                                       # name, environment, phase form
    ('no_group_gemm', {'COMIC_GROUP_GEMM': '0'}, False),
    ('no_persist', {'COMIC_PERSIST': '0'}, False),
    ('no_persist_bwd', {'COMIC_PERSIST_BWD': '0'}, False),
    ('no_fused_step', {'COMIC_FUSED_STEP': '0'}, False),
    ('one_lane', {'COMIC_GRAD_LANES': '0'}, False),
    ('no_split_attn_bwd', {'COMIC_SPLIT_ATTN_BWD': '0'}, False),
    ('exact_gemm', {'COMIC_SPLIT3': '0'}, False),
    ('phase_fwd_bwd', {}, True),
    # the switches that only show on a branch another switch selects: lanes without the grouped launches, the attention
    # backward's forms on the per-step chain, the per-step chains on two lanes, the own-rows backward loop
    ('no_group_gemm+one_lane', {'COMIC_GROUP_GEMM': '0', 'COMIC_GRAD_LANES': '0'}, False),
    ('no_persist_bwd+no_split_attn_bwd', {'COMIC_PERSIST_BWD': '0', 'COMIC_SPLIT_ATTN_BWD': '0'}, False),
    ('no_persist+no_group_gemm', {'COMIC_PERSIST': '0', 'COMIC_GROUP_GEMM': '0'}, False),
    ('no_fused_step+no_group_gemm', {'COMIC_FUSED_STEP': '0', 'COMIC_GROUP_GEMM': '0'}, False),
    ('bwd_own_rows', {'COMIC_BWD_OWN_ROWS': '1'}, False),
    ('no_group_gemm+phase_fwd_bwd', {'COMIC_GROUP_GEMM': '0'}, True),
]


def train_variants():
    tree = ast.parse(open(os.path.join(ROOT, 'tests', 'test_gpu_path.py')).read())
    node = next(n for n in tree.body if isinstance(n, ast.Assign) and n.targets[0].id == 'TRAIN_VARIANTS')
    return [{k.arg: ast.literal_eval(k.value) for k in e.keywords} for e in node.value.elts]      # a list of dict(...) calls


def batch(spec, B, L, seed):
    """Captions [B,L] (PAD = -1): row 0 is the longest and leaves one column of padding (T' = T - 1: the executor pads a step)."""
    rng = np.random.default_rng(seed)
    fm = rng.standard_normal((B, spec.M, spec.C)).astype(np.float32)
    im = rng.standard_normal((B, spec.Cg)).astype(np.float32)
    caps = np.full((B, L), -1, np.int64)
    for b in range(B):
        n = L - 3 if b == 0 else int(rng.integers(1, L - 2))
        caps[b, 0] = spec.start_id
        caps[b, 1:1 + n] = rng.integers(0, min(spec.V - 2, 256), n)
        caps[b, 1 + n] = spec.end_id
    return torch.from_numpy(fm).to(DEV), torch.from_numpy(im).to(DEV), caps


def params(spec, seed):
    p = cdec.init_params(spec, seed)
    rng = np.random.default_rng(seed + 100)
    for k in p:                                 # zero biases / unit gains would hide a gradient that is not written
        if p[k].ndim == 1:
            p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    return p


def digest(kw, B, L, phases, fields):
    spec = cdec.DecoderSpec(**dict(BASE, **kw))
    dec = cdec.Decoder(spec, params(spec, 3), DEV, seed=5)
    fm, im, caps = batch(spec, B, L, 7)
    rewards = np.random.default_rng(9).standard_normal(B).astype(np.float32)
    if phases:
        assert dec.train_step(fm, im, caps, training=True, seed=11, want_input_grads=True, phase='fwd') is None
        res = dec.train_step(None, None, caps, rewards=rewards, training=True, want_input_grads=True, phase='bwd')
    else:
        res = dec.train_step(fm, im, caps, rewards=rewards, training=True, seed=11, want_input_grads=True)
    torch.cuda.synchronize()
    paths = [dec.lib.comic_decoder_train_path()]
    parts = [(k, res[k]) for k in ('loss', 'map_loss', 'logits', 'ids', 'attn_maps')] + [
        ('grads', dec.grads.flat), ('dfm', res['dfm']), ('dim_embed', res['dim_embed'])]
    parts = [(k, v.detach().contiguous().cpu().numpy().tobytes()) for k, v in parts]
    sc = dec.score(fm, im, caps, want_attention=True)
    torch.cuda.synchronize()
    paths.append(dec.lib.comic_decoder_score_path())
    parts += [(k, sc[k].detach().contiguous().cpu().numpy().tobytes()) for k in ('token_log_probs', 'log_prob', 'attn_maps')]
    h = hashlib.sha256(repr(paths).encode())
    for _, b in parts:
        h.update(b)
    extra = ' ' + ' '.join('%s:%s' % (k, hashlib.sha256(b).hexdigest()[:8]) for k, b in parts) if fields else ''
    return 'train_path %d score_path %d sha256 %s%s' % (paths[0], paths[1], h.hexdigest(), extra)


def main():
    fields = '--fields' in sys.argv[1:]
    for i, kw in enumerate(train_variants()):
        print('variant%02d B=6 %s' % (i, digest(kw, 6, 12, False, fields)), flush=True)
    for B in (23, 64):
        line = digest(COMIC256, B, 12, False, fields)
        assert line.startswith('train_path 3 '), line             # both persistent loops
        print('comic256 B=%d %s' % (B, line), flush=True)
    for name, env, phases in SWITCHES:
        os.environ.update(env)
        try:
            print('comic256 B=64 %s %s' % (name, digest(COMIC256, 64, 12, phases, fields)), flush=True)
        finally:
            for k in env:
                del os.environ[k]


if __name__ == '__main__':
    main()
