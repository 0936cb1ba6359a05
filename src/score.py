#!/usr/bin/env python3
"""score.py -- log-likelihood and perplexity of GIVEN captions under a run's checkpoints.

Takes the arguments of infer.py that locate a run and its checkpoints, plus `--captions_file`: the JSON list of
`{image_id, caption}` that infer.py writes (`captions___N.json`); an image may appear several times (an n-best list).
The images are found as infer.py finds them (`--infer_set`, `--dataset_dir`).  Writes `scores___<checkpoint>.json`
beside the captions file: per entry `image_id`, `caption`, `log_prob` (natural log, summed over the tokens), `num_tokens`
and `perplexity = exp(-log_prob / num_tokens)`.  Forward only: CaptionModel.score_captions (comic_decoder_score)."""
import argparse
import json
import math
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')      # before the HIP runtime initialises: see comic_amd/__init__.py

CURR_DIR = os.path.dirname(os.path.realpath(__file__))
BASE_DIR = os.path.dirname(CURR_DIR)
sys.path.insert(0, BASE_DIR)
pjoin = os.path.join


def create_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    a('--captions_file', type=str, required=True,
      help='JSON list of {image_id, caption} (the `captions___N.json` of infer.py) to be scored.')
    a('--infer_set', type=str, default='test', choices=['test', 'valid', 'coco_test', 'coco_valid'],
      help='The split the captions belong to.')
    a('--infer_checkpoints_dir', type=str, default=pjoin('mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01'),
      help='The directory containing the checkpoint files.')
    a('--infer_checkpoints', type=str, default='all', help='The checkpoint numbers to score with. Comma-separated.')
    a('--dataset_dir', type=str, default=pjoin(BASE_DIR, 'datasets', 'mscoco'), help='Dataset directory.')
    a('--gpu', type=str, default='0', help='The gpu number.')
    a('--batch_size_infer', type=int, default=25, help='The batch size.')
    a('--loader_split_jpeg', action=argparse.BooleanOptionalAction, default=None,
      help='Split JPEG decode: C threads undo the entropy coding, the device does the pixels (bit-identical to PIL).')
    a('--loader_threads', type=int, default=None, help='Decode threads of the loader.')
    a('--loader_cache_gb', type=float, default=None, help='Coefficient cache of the split JPEG decoder, GB.')
    a('--cnn_dtype', type=str, default=None, choices=['bf16', 'f16', 'f32', 'bf16x3'],
      help='CNN plan of the scoring run (default: the training run\'s), as in infer.py.')
    a('--infer_ema', action='store_true', default=None,
      help='Score with the averaged weights of a run trained with --ema_decay (`model_ema-N`), as in infer.py.')
    return p


def find_checkpoints(ckpt_dir, which, prefix='model_compact-'):
    """infer.py's checkpoint discovery: 'all' -> every `model_compact-N.npz` / `.index` of the directory."""
    from comic_amd.configuration import natural_keys
    if which != 'all':
        return [n for n in which.split(',') if n]
    files = [f[len(prefix):].rsplit('.', 1)[0] for f in sorted(os.listdir(ckpt_dir), key=natural_keys)
             if f.startswith(prefix) and (f.endswith('.npz') or f.endswith('.index'))]
    files = sorted(set(files), key=natural_keys)
    return files[-12:] if len(files) > 20 else files


def image_id_of(filename):
    """The image id infer.py writes for an image file (infer_fn.py: COCO number, or the base name of an `@` path)."""
    import re
    image_id = filename.replace('.jpg', '')
    if '@' in image_id:
        return os.path.basename(image_id)
    found = re.findall(r'(?<=_)\d+', image_id)
    if not found:
        raise ValueError('cannot derive an image id from `{}`'.format(filename))
    return int(found[0])


def tokenise(captions, config, radix_wtoi=None):
    """Caption strings -> padded id matrix [N, L] (<GO> ... <EOS>, PAD = -1) with the run's vocabulary."""
    from comic_amd.ops import captions_to_batched_ids
    return captions_to_batched_ids([[c] for c in captions], config, radix_wtoi)


def make_record(entry, log_prob, num_tokens):
    log_prob, num_tokens = float(log_prob), int(num_tokens)
    return dict(image_id=entry['image_id'], caption=entry['caption'], log_prob=log_prob, num_tokens=num_tokens,
                perplexity=math.exp(-log_prob / max(num_tokens, 1)))


def score_entries(entries, filenames, image_batches, batch_size, config, scorer, radix_wtoi=None):
    """Scores every entry whose image is among `filenames` (consumed batch by batch from `image_batches`, in order).
    scorer(images, ids [n,L]) -> (log_prob [n], lengths [n]).  An image with k entries is scored in k rounds.
    -> records in the order of `entries`; an entry whose image was not met raises."""
    by_image = {}
    for i, e in enumerate(entries):
        by_image.setdefault(str(e['image_id']), []).append(i)
    records = [None] * len(entries)
    for step in range(len(filenames) // batch_size):
        batch = next(image_batches)
        images = batch[0] if isinstance(batch, (tuple, list)) else batch
        names = filenames[step * batch_size:(step + 1) * batch_size]
        wanted = [by_image.get(str(image_id_of(f)), []) for f in names]
        for k in range(max((len(w) for w in wanted), default=0)):
            rows = [r for r, w in enumerate(wanted) if len(w) > k]
            idx = [wanted[r][k] for r in rows]
            ids = tokenise([entries[i]['caption'] for i in idx], config, radix_wtoi)
            logp, lens = scorer(images[rows], ids)
            for i, lp, n in zip(idx, logp, lens):
                records[i] = make_record(entries[i], lp, n)
    missing = [entries[i]['image_id'] for i, r in enumerate(records) if r is None]
    if missing:
        raise ValueError('no image of the split for image ids {} ...'.format(missing[:5]))
    return records


def score_checkpoint(config, ckpt_path, entries, device='cuda:0'):
    from comic_amd import inputs, model as mdl
    mdl.reset_default_graph()
    inputs_man = inputs.InputManager(config, is_inference=True)
    try:
        inputs_man.enable_device_preprocess(device)
        c = inputs_man.config
        c.checkpoint_path, c.resume_training = ckpt_path, False
        m = mdl.CaptionModel(c, mode='infer', batch_ops=inputs_man.batch_infer, reuse=False, name='scoring', device=device)
        m.restore_model()

        def scorer(images, ids):
            res = m.score_captions(images, ids)
            return res['log_prob'].cpu().numpy(), res['lengths'].numpy()
        return score_entries(entries, inputs_man.filenames_infer, inputs_man.batch_infer, c.batch_size_infer, c, scorer,
                             getattr(inputs_man, 'radix_wtoi', None))
    finally:
        inputs_man.close()


def main(argv=None):
    from comic_amd import configuration as conf
    args = create_parser().parse_args(argv)
    if not os.path.isabs(args.infer_checkpoints_dir):
        args.infer_checkpoints_dir = pjoin(BASE_DIR, 'experiments', args.infer_checkpoints_dir)
    prefix = 'model_ema-' if args.infer_ema else 'model_compact-'
    if args.infer_ema and not any(f.startswith(prefix) for f in os.listdir(args.infer_checkpoints_dir)):
        raise ValueError('--infer_ema: `{}` holds no `model_ema-*` checkpoint: train the run with --ema_decay'.format(
            args.infer_checkpoints_dir))
    ckpts = find_checkpoints(args.infer_checkpoints_dir, args.infer_checkpoints, prefix)
    with open(args.captions_file) as f:
        entries = json.load(f)
    c = conf.load_config(pjoin(args.infer_checkpoints_dir, 'config.pkl'))
    c.__dict__.update({k: v for k, v in args.__dict__.items() if v is not None})
    import torch
    torch.cuda.set_device(int(str(c.gpu).split(',')[0]))
    for n in ckpts:
        path = pjoin(c.infer_checkpoints_dir, prefix + n)
        if not (os.path.isfile(path) or os.path.isfile(path + '.npz') or os.path.isfile(path + '.index')):
            print('WARNING: `{}` not found. Checkpoint skipped.'.format(os.path.basename(path)))
            continue
        records = score_checkpoint(c, path, entries)
        out = pjoin(os.path.dirname(os.path.abspath(args.captions_file)), 'scores___{}.json'.format(n))
        with open(out, 'w') as f:
            json.dump(records, f)
        print('INFO: {} captions scored with checkpoint {}: mean perplexity {:.3f} -> {}'.format(
            len(records), n, sum(r['perplexity'] for r in records) / max(len(records), 1), out))


if __name__ == '__main__':
    main()
