#!/usr/bin/env python3
"""infer.py -- same flags, checkpoint discovery, `config.pkl` overlay and output directory
naming as the reference CLI (reference src/infer.py:23-141)."""
import argparse
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
    a('--infer_set', type=str, default='test', choices=['test', 'valid', 'coco_test', 'coco_valid'],
      help='The split to perform inference on.')
    a('--infer_checkpoints_dir', type=str, default=pjoin('mscoco', 'radix_b256_add_LN_softmax_h8_tie_lstm_run_01'),
      help='The directory containing the checkpoint files.')
    a('--infer_checkpoints', type=str, default='all', help='The checkpoint numbers to be evaluated. Comma-separated.')
    a('--annotations_file', type=str, default='captions_val2014.json',
      help='The annotations / reference file for calculating scores.')
    a('--dataset_dir', type=str, default=pjoin(BASE_DIR, 'datasets', 'mscoco'), help='Dataset directory.')
    a('--run_inference', type=bool, default=True, help='Whether to perform inference.')
    a('--get_metric_score', type=bool, default=True, help='Whether to perform metric score calculations.')
    a('--save_attention_maps', type=bool, default=False, help='Whether to save attention maps to disk as pickle file.')
    a('--gpu', type=str, default='0', help='The gpu number.')
    a('--per_process_gpu_memory_fraction', type=float, default=0.75, help='The fraction of GPU memory allocated.')
    a('--infer_beam_size', type=int, default=3, help='The beam size.')
    a('--infer_length_penalty_weight', type=float, default=0.0, help='The length penalty weight used in beam search.')
    a('--infer_max_length', type=int, default=30, help='The maximum caption length allowed during inference.')
    a('--batch_size_infer', type=int, default=25, help='The batch size.')
    # additions of this framework (the training run's choices apply when left out)
    a('--loader_split_jpeg', action=argparse.BooleanOptionalAction, default=None,
      help='Split JPEG decode: C threads undo the entropy coding, the device does the pixels (bit-identical to PIL).')
    a('--loader_threads', type=int, default=None, help='Decode threads of the loader.')
    a('--loader_cache_gb', type=float, default=None, help='Coefficient cache of the split JPEG decoder, GB.')
    a('--cnn_dtype', type=str, default=None, choices=['bf16', 'f16', 'f32', 'bf16x3'],
      help='CNN plan of the inference run (default: the training run\'s).  Checkpoints hold fp32 variables, so any '
           'run decodes on any plan, e.g. a bf16-trained model on f16.')
    a('--infer_ensemble', action='store_true', default=None,
      help='Decode the checkpoints of --infer_checkpoints TOGETHER: one beam search over the mean of their word '
           'distributions; writes captions___ens_<n1>+<n2>+....json.')
    a('--infer_ensemble_weights', type=str, default=None,
      help='Comma-separated weights of the ensemble members (>= 0, summing to 1; default uniform).')
    a('--infer_min_length', type=int, default=None,
      help='Beam search: no caption ends before this many words (characters with char tokens).')
    a('--infer_no_repeat_ngram', type=int, default=None,
      help='Beam search: no n-gram of this many words (characters with char tokens) occurs twice in a caption.')
    a('--infer_suppress_words', type=str, default=None,
      help='Beam search: comma-separated words that are never emitted, e.g. `<UNK>` (word and char tokens only).')
    a('--infer_beam_groups', type=int, default=None,
      help='Diverse beam search: split the beam into this many groups (infer_beam_size must be a multiple); also writes '
           'caption_groups___N.json with the best caption of every group.')
    a('--infer_diversity', type=float, default=None,
      help='Diverse beam search: the Hamming diversity penalty a later group pays per earlier pick of the same token.')
    a('--infer_sample', action='store_true', default=None,
      help='Sample --infer_beam_size captions per image instead of beam search; captions___N.json keeps, per image, the '
           'sample of highest log-probability, caption_samples___N.json every sample with its log-probability.')
    a('--infer_temperature', type=float, default=None, help='Sampling: the temperature of the word distribution (default 1).')
    a('--infer_sample_seed', type=int, default=None, help='Sampling: the seed of the noise generator (default 0).')
    a('--infer_top_k', type=int, default=None,
      help='Sampling: draw every token from the k likeliest only (0 = off; needs --infer_sample).')
    a('--infer_top_p', type=float, default=None,
      help='Sampling: draw every token from the smallest set of likeliest tokens whose probability reaches p (the nucleus; '
           'after --infer_top_k; 1 = off; needs --infer_sample).')
    a('--infer_consensus', action='store_true', default=None,
      help='Sampling: captions___N.json keeps, per image, the sample that agrees most with its siblings (their mean '
           'CIDEr-D similarity, computed on the device) instead of the likeliest; caption_samples___N.json gains every '
           'sample\'s `consensus`.  Needs --infer_sample; word and radix tokens; output goes to `..._cns`.')
    a('--infer_consensus_df', type=str, default=None,
      help='Consensus: the `{pattern}scst-words.p` document-frequency pickle of scst/prepro_ngrams.py for the idf weights of '
           'the n-grams (without it every n-gram weighs 1); output goes to `..._cns_df`.  Needs --infer_consensus.')
    a('--infer_require_file', type=str, default=None,
      help='Beam search with required words: a JSON file of image file name or image_id -> list of words the caption has '
           'to contain (word and radix tokens); also writes caption_required___N.json with the words met and every '
           'non-empty bank\'s best caption.  --infer_beam_size must be a multiple of words * tokens per word + 1.')
    a('--infer_require_words', type=int, default=None,
      help='Required words per image, 1 to 4 (default: the longest list in the file, at most 4); further words are dropped.')
    a('--infer_prefix', type=str, default=None,
      help='Forced-prefix decoding: every caption starts with these words, e.g. "a close up of" (word and radix tokens; a '
           'word outside the vocabulary is an error); also writes caption_prefix___N.json with the caption\'s log_prob and '
           'prefix_log_prob; output goes to `..._pfx_<words joined by ->`.  Not together with --infer_prefix_file.')
    a('--infer_prefix_file', type=str, default=None,
      help='Forced-prefix decoding per image: a JSON file of image file name or image_id -> string or list of words the '
           'caption starts with; a prefix is cut before its first word outside the vocabulary (reported in '
           'caption_prefix___N.json); output goes to `..._pfx_<file stem>`.')
    a('--infer_ema', action='store_true', default=None,
      help='Decode the averaged weights of a run trained with --ema_decay: the `model_ema-N` checkpoints instead of '
           '`model_compact-N`; output goes to a directory of its own (`..._ema`).')
    a('--infer_average', action='store_true', default=None,
      help='Average the variables of the (at least two) checkpoints of --infer_checkpoints into ONE model and decode that; '
           'output goes to `..._avg_<n1>+<n2>+...`.  Not together with --infer_ensemble.')
    return p


def checkpoint_prefix(args):
    """`model_compact-`, or `model_ema-` with --infer_ema (train.py --ema_decay writes both, with the same variables)."""
    return 'model_ema-' if getattr(args, 'infer_ema', None) else 'model_compact-'


def ema_dir_suffix(args):
    return '_ema' if getattr(args, 'infer_ema', None) else ''


def average_dir_suffix(args):
    if not getattr(args, 'infer_average', None):
        return ''
    return '_avg_' + '+'.join(str(n) for n in args.infer_checkpoints)


def check_weight_averaging(args, files=None):
    """Refusals of --infer_ema / --infer_average, before anything is loaded.  args.infer_checkpoints: the list of numbers;
    files: the names in the run directory (None: not looked at)."""
    if getattr(args, 'infer_ema', None) and files is not None and not any(f.startswith('model_ema-') for f in files):
        raise ValueError('--infer_ema: `{}` holds no `model_ema-*` checkpoint: train the run with --ema_decay'.format(
            args.infer_checkpoints_dir))
    if getattr(args, 'infer_average', None):
        if getattr(args, 'infer_ensemble', None):
            raise ValueError('--infer_average builds one model, --infer_ensemble decodes several: choose one')
        if len(args.infer_checkpoints) < 2:
            raise ValueError('--infer_average needs at least two --infer_checkpoints, got {}'.format(
                ','.join(args.infer_checkpoints) or 'none'))


def _ckpt_path(directory, ckpt_prefix, ckpt_num):
    path = pjoin(directory, ckpt_prefix + ckpt_num)
    return path + '.npz' if os.path.isfile(path + '.npz') else path       # else: TF bundle prefix


def write_average(c, ckpt_prefix):
    """--infer_average: the mean of the listed checkpoints, written into the output directory as a compact `.npz`
    checkpoint numbered like the last of them -- what the single-checkpoint path then decodes (and a checkpoint like any
    other: beside a config.pkl every consumer of `model_compact-N` reads it).  Returns (path, number)."""
    from comic_amd import checkpoint as ckpt
    import numpy as np
    num = c.infer_checkpoints[-1]
    path = pjoin(c.infer_save_path, 'model_compact-{}.npz'.format(num))
    if not os.path.isfile(path):
        mean = ckpt.average_variables(ckpt.load(_ckpt_path(c.infer_checkpoints_dir, ckpt_prefix, n))
                                      for n in c.infer_checkpoints)
        np.savez(path, **mean)
    return path, num


def main(argv=None):
    from comic_amd import configuration as conf, infer_fn as infer
    from comic_amd.configuration import natural_keys
    args = create_parser().parse_args(argv)
    ckpt_prefix = checkpoint_prefix(args)
    if not os.path.isabs(args.infer_checkpoints_dir):
        args.infer_checkpoints_dir = pjoin(BASE_DIR, 'experiments', args.infer_checkpoints_dir)
    if args.infer_checkpoints == 'all':
        files = sorted(os.listdir(args.infer_checkpoints_dir), key=natural_keys)
        # `.npz` containers and TF tensor bundles (`model_compact-N.index`, like the reference's own)
        files = [f[len(ckpt_prefix):].rsplit('.', 1)[0] for f in files
                 if f.startswith(ckpt_prefix) and (f.endswith('.npz') or f.endswith('.index'))]
        files = sorted(set(files), key=natural_keys)
        if len(files) > 20:
            files = files[-12:]
        args.infer_checkpoints = files
    else:
        args.infer_checkpoints = args.infer_checkpoints.split(',')
        if len(args.infer_checkpoints) < 1:
            raise ValueError('`infer_checkpoints` must be either `all` or a list of comma-separated checkpoint numbers.')
    check_weight_averaging(args, os.listdir(args.infer_checkpoints_dir) if os.path.isdir(args.infer_checkpoints_dir) else None)
    c = conf.load_config(pjoin(args.infer_checkpoints_dir, 'config.pkl'))
    c.__dict__.update({k: v for k, v in args.__dict__.items() if v is not None})
    save_name = 'beam_{}_lpen_{}'.format(c.infer_beam_size, c.infer_length_penalty_weight)
    save_name = {'test': 'infer_test_', 'valid': 'infer_valid_', 'coco_test': 'infer_cocoTest_',
                 'coco_valid': 'infer_cocoValid_'}[c.infer_set] + save_name
    # constrained, grouped and sampled captions get a directory of their own: they never overwrite the plain ones
    from comic_amd.decoder import decode_dir_suffix, options_from_config
    # refused before anything is loaded: groups that do not divide infer_beam_size; sampling with more than one group or a
    # length penalty; --infer_top_k / --infer_top_p or --infer_consensus without --infer_sample; required words or a consensus
    # on char tokens; a beam size that the banks of the required words do not divide; --infer_prefix with --infer_prefix_file,
    # on char tokens or with a word outside the vocabulary
    options_from_config(c, load=False)
    save_name += decode_dir_suffix(c)
    save_name += ema_dir_suffix(c) + average_dir_suffix(c)      # averaged weights never overwrite the plain captions either
    c.infer_save_path = pjoin(c.infer_checkpoints_dir, save_name)
    if os.path.exists(c.infer_save_path):
        print('\nINFO: `eval_log_path` already exists.')
    else:
        print('\nINFO: `eval_log_path` will be created.')
        os.mkdir(c.infer_save_path)
    import torch
    torch.cuda.set_device(int(str(c.gpu).split(',')[0]))
    scores_combined = {}
    if getattr(c, 'infer_ensemble', None):
        return run_ensemble(c, ckpt_prefix)
    averaged = write_average(c, ckpt_prefix) if getattr(c, 'infer_average', None) else None
    for ckpt_num in ([averaged[1]] if averaged else c.infer_checkpoints):
        path = averaged[0] if averaged else _ckpt_path(c.infer_checkpoints_dir, ckpt_prefix, ckpt_num)
        # metric scores: the native BLEU / ROUGE-L / CIDEr scorers when the annotation file is there (the reference
        # shells out to the Java COCO toolkit for METEOR / SPICE / PTB tokenisation as well, infer_fn.py:295-315)
        ann = c.annotations_file if os.path.isabs(c.annotations_file) else pjoin(c.dataset_dir, 'captions', c.annotations_file)
        evaluator = None
        if c.get_metric_score and os.path.isfile(ann):
            from comic_amd import coco_eval
            c.annotations_file = ann
            evaluator = coco_eval.evaluate_captions
        elif c.get_metric_score:
            print('INFO: annotation file `{}` not found: captions are written, metric scores skipped.'.format(ann))
        infer.evaluate_model(config=c, curr_ckpt_path=path, scores_combined=scores_combined, evaluate_captions=evaluator)
        print('\n')


def run_ensemble(c, ckpt_prefix):
    """--infer_ensemble: the listed checkpoints as one ensemble; metric scores through the same hand-off."""
    from comic_amd import infer_fn as infer
    paths = []
    for ckpt_num in c.infer_checkpoints:
        paths.append(_ckpt_path(c.infer_checkpoints_dir, ckpt_prefix, ckpt_num))
    weights = None
    if getattr(c, 'infer_ensemble_weights', None):
        weights = [float(w) for w in str(c.infer_ensemble_weights).split(',')]
    tag = infer.ensemble_name(c.infer_checkpoints)
    coco_json = pjoin(c.infer_save_path, 'captions___{}.json'.format(tag))
    if c.run_inference:
        if os.path.isfile(coco_json):
            print('INFO: Found caption file `{}`. Skipping inference.'.format(os.path.basename(coco_json)))
        else:
            infer.run_inference_ensemble(c, paths, weights)
    ann = c.annotations_file if os.path.isabs(c.annotations_file) else pjoin(c.dataset_dir, 'captions', c.annotations_file)
    if c.get_metric_score and os.path.isfile(ann):
        from comic_amd import coco_eval
        results = coco_eval.evaluate_captions(ann, coco_json)
        metrics = [m for m in ['Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr', 'SPICE'] if m in results]
        with open(pjoin(c.infer_save_path, 'metric_scores.txt'), 'a', newline='') as f:
            f.write('===================================\r\n%s\r\nBeam size: %d\r\n===================================\r\n'
                    % (tag, c.infer_beam_size))
            f.write('\r\n'.join('{}: {:1.3f}'.format(m, results[m]) for m in metrics) + '\r\n\r\n\r\n')
    elif c.get_metric_score:
        print('INFO: annotation file `{}` not found: captions are written, metric scores skipped.'.format(ann))


if __name__ == '__main__':
    main()
