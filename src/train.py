#!/usr/bin/env python3
"""train.py -- same flags, mode chaining, run-directory naming and kwargs as the reference
CLI (reference src/train.py:25-312), driving the MI355X-native path.

Differences (all additive): `--cnn_dtype {bf16,f16,f32,bf16x3}`, `--checkpoint_format {npz,tf}`, `--ema_decay`, `--prune_*`, `--label_smoothing`,
`--distill_checkpoints / _weight / _top_k / _temperature / _weights`,
`--cnn_input_augment_crop {fixed,area}`, `--cnn_input_augment_area_min`, `--cnn_input_augment_color {none,fast,full}`; launched under
`python -m torch.distributed.run --nproc-per-node N` it trains data-parallel (one process
per GPU, RCCL gradient all-reduce); the slim checkpoint is not downloaded (no network):
pass `--checkpoint_path` (an .npz with slim variable names) or train the CNN from random init.
"""
import argparse
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')      # before the HIP runtime initialises: see comic_amd/__init__.py

CURR_DIR = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, os.path.dirname(CURR_DIR))
pjoin = os.path.join


def create_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    a('--name', type=str, default='lstm', help='The logging name.')
    a('--dataset_dir', type=str, default='', help='The dataset directory.')
    a('--dataset_file_pattern', type=str, default='mscoco_{}_w5_s20_include_restval',
      help='The dataset text files naming pattern.')
    a('--train_mode', type=str, default='decoder', choices=['decoder', 'cnn_finetune', 'scst'],
      help='Str. The training regime.')
    a('--legacy', type=bool, default=False, help='If True, will match settings as described in paper.')
    a('--token_type', type=str, default='radix', choices=['radix', 'word', 'char'], help='The language model.')
    a('--radix_base', type=int, default=256, help='The base for Radix models.')
    a('--cnn_name', type=str, default='inception_v1', help='The CNN model name.')
    a('--cnn_input_size', type=str, default='224,224', help='The network input size.')
    a('--cnn_input_augment', type=bool, default=True, help='Whether to augment input images.')
    a('--cnn_input_augment_crop', type=str, default='fixed', choices=['fixed', 'area'],
      help='Crop of the training images: `fixed`: the 224 window of the 256 x 256 resize (the reference); `area`: a box of random '
           'area and aspect ratio (3/4 ... 4/3) cut from the source image and resized straight to the input size, on the device; '
           'the run directory gets `_augA<area_min>`.')
    a('--cnn_input_augment_area_min', type=float, default=0.35,
      help='With --cnn_input_augment_crop area: the smallest share of the image a box covers, in (0, 1].')
    a('--cnn_input_augment_color', type=str, default='none', choices=['none', 'fast', 'full'],
      help='Colour distortion of the training images (slim distort_color), on the device: `fast` brightness and saturation, '
           '`full` brightness, saturation, hue and contrast, in an order drawn per image; the run directory gets `_augC<mode>`.')
    a('--cnn_fm_attention', type=str, default='Mixed_4f', help='String, name of feature map for attention.')
    a('--cnn_fm_projection', type=str, default='tied', choices=['none', 'independent', 'tied'],
      help='String, feature map projection, from `none`, `independent`, `tied`.')
    a('--rnn_name', type=str, default='LSTM', choices=['LSTM', 'LN_LSTM', 'GRU'],
      help='The type of RNN, from `LSTM`, `LN_LSTM` and `GRU`.')
    a('--rnn_size', type=int, default=512, help='Int, number of RNN units.')
    a('--rnn_word_size', type=int, default=256, help='The word size.')
    a('--rnn_init_method', type=str, default='first_input', choices=['project_hidden', 'first_input'],
      help='The RNN init method.')
    a('--rnn_recurr_dropout', type=bool, default=False, help='Whether to enable variational recurrent dropout.')
    a('--attn_num_heads', type=int, default=8, help='The number of attention heads.')
    a('--attn_context_layer', type=bool, default=False,
      help='If True, add linear projection after multi-head attention.')
    a('--attn_alignment_method', type=str, default='add_LN', choices=['add_LN', 'add', 'dot'],
      help='Str, The alignment method / composition method.')
    a('--attn_probability_fn', type=str, default='softmax', choices=['softmax', 'sigmoid'],
      help='Str, The attention map probability function.')
    a('--attn_keep_prob', type=float, default=0.9, help='Float, The keep rate for attention map dropout.')
    a('--initialiser', type=str, default='xavier', choices=['xavier', 'he', 'none'],
      help='The initialiser: `xavier`, `he`, tensorflow default.')
    a('--optimiser', type=str, default='adam', choices=['adam', 'sgd'], help='The optimiser: `adam`, `sgd`.')
    a('--batch_size_train', type=int, default=32, help='The batch size for training.')
    a('--batch_size_eval', type=int, default=61, help='The batch size for validation.')
    a('--max_epoch', type=int, default=30, help='The max epoch training.')
    a('--lr_start', type=float, default=1e-2, help='Float, determines the starting learning rate.')
    a('--lr_end', type=float, default=1e-5, help='Float, determines the ending learning rate.')
    a('--cnn_grad_multiplier', type=float, default=1.0,
      help='Float, determines the gradient multiplier when back-prop thru CNN.')
    a('--adam_epsilon', type=float, default=1e-2, help='Float, determines the epsilon value of ADAM.')
    a('--scst_beam_size', type=int, default=7, help='The beam size for SCST sampling.')
    a('--scst_weight_ciderD', type=float, default=1.0, help='The weight for CIDEr-D metric during SCST training.')
    a('--scst_weight_bleu', type=str, default='0,0,0,2', help='The weight for BLEU metrics during SCST training.')
    a('--scst_rollout', type=str, default='beam', choices=['beam', 'sample'],
      help='SCST rollouts: `beam` search, or `sample`: scst_beam_size independent samples per image, drawn on the device.')
    a('--scst_temperature', type=float, default=1.0, help='Temperature of the sampled SCST rollouts.')
    a('--scst_baseline', type=str, default='greedy', choices=['greedy', 'mean'],
      help='SCST baseline: the reward of the `greedy` rollout, or `mean`: the mean reward of the image\'s other rollouts '
           '(leave-one-out; no greedy rollout is decoded; needs --scst_beam_size >= 2).')
    a('--scst_reward', type=str, default='host', choices=['host', 'device'],
      help='Where the SCST reward is formed: the `host` scorer on text, or one launch on the `device` (word / radix tokens).')
    a('--freeze_scopes', type=str, default='Model/encoder/cnn', help='The scopes to freeze / do not train.')
    a('--checkpoint_path', type=str, default=None, help='The checkpoint path.')
    a('--checkpoint_exclude_scopes', type=str, default='', help='The scopes to exclude when restoring from checkpoint.')
    a('--gpu', type=str, default='0', help='The gpu number.')
    a('--run', type=int, default=1, help='The run number.')
    # additions of this framework
    a('--cnn_dtype', type=str, default='bf16', choices=['bf16', 'f16', 'f32', 'bf16x3'],
      help='CNN activation / MFMA input type.  f16: IEEE half activations and filters on the f16 matrix cores (bf16 '
           'speed, about 7x closer to fp32; frozen-CNN modes only: decoder, scst, infer).  bf16x3: hi/lo-split '
           'activations and filters on the bf16 matrix cores (fp32-class accuracy).')
    a('--checkpoint_format', type=str, default='npz', choices=['npz', 'tf'],
      help='Container of saved checkpoints: .npz or the TF checkpoint-V2 tensor bundle (both restore).')
    a('--log_root', type=str, default='', help='Root of the experiments directory (default: ../experiments).')
    a('--encoder_group', type=int, default=0,
      help='Frozen-CNN modes: training steps served by ONE encoder forward (group x batch images per forward, on a '
           'second stream under the decoder steps). 0 = auto (about 1280 images per forward), 1 = one forward per step.')
    a('--loader_processes', type=int, default=0,
      help='JPEG decode in this many worker processes (shared-memory staging); 0 = decode threads in this process.')
    a('--loader_split_jpeg', action=argparse.BooleanOptionalAction, default=True,
      help='Split JPEG decode (default): `loader_threads` C threads undo the entropy coding, the device does inverse DCT / '
           'upsampling / colour conversion (bit-identical to PIL); files it does not take (progressive, CMYK, PNG) go through PIL.  '
           '--no-loader_split_jpeg: PIL decode on threads / --loader_processes.')
    a('--loader_threads', type=int, default=0, help='Decode threads of the loader (0 = min(16, cores)).')
    a('--loader_cache_gb', type=float, default=0.0,
      help='With --loader_split_jpeg: keep the decoded DCT coefficients of the images in host memory (as their non-zeros: about the '
           'size of the JPEG files) up to this many GB; the epochs after the first skip file reads and Huffman decoding.')
    a('--ema_decay', type=float, default=0.0,
      help='Keep an exponential moving average of every trained variable (tf.train.ExponentialMovingAverage with '
           'num_updates: decay min(d, (1 + n) / (10 + n))), updated inside the optimiser launch; `model_ema-N` is written '
           'beside `model_compact-N` (infer.py / score.py --infer_ema).  0 = off, else in (0, 1).')
    a('--label_smoothing', type=float, default=0.0,
      help='Label smoothing of the XE loss (decoder / cnn_finetune): this share of every target is spread uniformly over the '
           'vocabulary.  0 = off, else in (0, 1).')
    a('--distill_checkpoints', type=str, default='',
      help='Distil teacher checkpoint(s) into this model (--train_mode decoder): p1[,p2...], `model_compact-N` / `model_ema-N` '
           'paths, each with the config.pkl of its run beside it; several teach as an ensemble.')
    a('--distill_weight', type=float, default=0.0,
      help='Share of every target taken from the teacher, in (0, 1]; label_smoothing + distill_weight <= 1.')
    a('--distill_top_k', type=int, default=16, help='Entries of the teacher distribution kept per token (1 ... 32).')
    a('--distill_temperature', type=float, default=1.0, help='Temperature of the teacher softmax.')
    a('--distill_weights', type=str, default='', help='Weights w1,... of several teachers (>= 0, summing to 1; default uniform).')
    a('--prune_sparsity', type=float, default=0.0,
      help='Gradual magnitude pruning (Zhu & Gupta 2017) of the decoder\'s weight matrices towards this share of zeros, the '
           'masks chosen and kept on the device; the run directory gets `_pr<s>` (`_pr<s>g` for --prune_scope global).  '
           '0 = off, else in (0, 1).')
    a('--prune_start_step', type=int, default=-1, help='First mask event (default: 10 %% of the run\'s steps).')
    a('--prune_end_step', type=int, default=-1,
      help='Last mask event, where --prune_sparsity is reached (default: 60 %% of the run\'s steps, moved down to a multiple of '
           '--prune_every behind the start; given, it must be one).')
    a('--prune_every', type=int, default=100, help='Optimiser updates between two mask events.')
    a('--prune_scope', type=str, default='layer', choices=['layer', 'global'],
      help='`layer`: every variable reaches the sparsity on its own; `global`: the smallest weights of all prunable variables '
           'together.')
    a('--prune_variables', type=str, default='',
      help='Comma list of the decoder variables to prune (default: every one with two dimensions: W_init, K, K_c, W_m, W_v, '
           'W_q, W_a, W_o, emb, where present).')
    a('--prune_keep_zeros', action='store_true',
      help='A later stage on a pruned checkpoint: the zeros of the prunable variables as loaded stay zero (a frozen mask, no '
           'schedule; not with --prune_sparsity).')
    return p


def build_kwargs(args):
    """Everything between argument parsing and `try_to_train` in the reference (train.py:167-302)."""
    args.cnn_input_size = [int(v) for v in str(args.cnn_input_size).split(',')]
    if args.legacy:
        print('LEGACY mode enabled. Some arguments will be overridden.')
        args.__dict__.update(cnn_name='inception_v1', cnn_input_size=[224, 224], cnn_input_augment=True,
                             cnn_fm_attention='Mixed_4f', rnn_name='LSTM', rnn_size=512, rnn_word_size=256,
                             rnn_init_method='project_hidden', rnn_recurr_dropout=False, attn_context_layer=False,
                             attn_alignment_method='add_LN', attn_probability_fn='softmax', attn_keep_prob=1.0,
                             lr_start=1e-3, lr_end=2e-4, lr_reduce_every_n_epochs=4, cnn_grad_multiplier=1.0,
                             initialiser='xavier', optimiser='adam', batch_size_train=32, adam_epsilon=1e-6)
    rand_seed = {1: 48964896, 2: 88888888, 3: 123456789}[args.run]
    dataset = args.dataset_file_pattern.split('_')[0]
    log_root = args.log_root or pjoin(os.path.dirname(CURR_DIR), 'experiments', dataset)
    if args.log_root:
        log_root = pjoin(args.log_root, dataset)
    if args.dataset_dir == '':
        args.dataset_dir = pjoin(os.path.dirname(CURR_DIR), 'datasets', dataset)
    token = 'radix_b{}'.format(args.radix_base) if args.token_type == 'radix' else args.token_type
    name = '_'.join([token, args.attn_alignment_method, args.attn_probability_fn,
                     'h{}'.format(args.attn_num_heads), args.cnn_fm_projection[:3], args.name])
    if args.legacy:
        name = 'legacy_' + name
    # a soft-target run gets a directory of its own: `_ls<eps>` for both XE modes (cnn_finetune continues the decoder run
    # of the same --label_smoothing), `_kd<weight>_k<K>_t<temperature>` for a distilled decoder run
    smooth, distil = soft_dir_suffixes(args)
    # a pruned run likewise, `_pr<s>[g]` right behind the name -- of the stage that prunes only: it starts from the
    # checkpoint of the plain earlier stage, and a later stage names the pruned one by `--name <name>_pr<s>`
    from comic_amd import augment, prune
    # ... and one with --cnn_input_augment_crop area / --cnn_input_augment_color, `_aug[A<area_min>][C<mode>]`
    pruned = name + prune.dir_suffix(args) + augment.dir_suffix(args)
    dec_dir = pjoin(log_root, '{}{}_run_{:02d}'.format(name, smooth, args.run))
    cnnft_dir = pjoin(log_root, '{}{}_cnnFT_run_{:02d}'.format(name, smooth, args.run))
    train_fn_name = 'train_fn'
    if args.train_mode == 'decoder':
        assert args.freeze_scopes == 'Model/encoder/cnn'
        log_path = pjoin(log_root, '{}{}{}_run_{:02d}'.format(pruned, smooth, distil, args.run))
    elif args.train_mode == 'cnn_finetune':
        if args.legacy:
            raise NotImplementedError
        if not os.path.exists(dec_dir):
            raise ValueError('Decoder training log path not found: {}'.format(dec_dir))
        args.lr_start, args.max_epoch, args.freeze_scopes, args.checkpoint_path = 1e-3, 10, '', dec_dir
        log_path = pjoin(log_root, '{}{}_cnnFT_run_{:02d}'.format(pruned, smooth, args.run))
    else:
        if args.legacy:
            raise NotImplementedError
        if not os.path.exists(cnnft_dir):
            raise ValueError('CNN finetune log path not found: {}'.format(cnnft_dir))
        args.scst_weight_bleu = [float(w) for w in args.scst_weight_bleu.split(',')]
        args.batch_size_train, args.lr_start, args.max_epoch = 10, 1e-3, 10
        args.freeze_scopes, args.checkpoint_path = 'Model/encoder/cnn', cnnft_dir
        scst = 'beam_{}_CrD_{}_B1_{}_B4_{}'.format(args.scst_beam_size, args.scst_weight_ciderD,
                                                   args.scst_weight_bleu[0], args.scst_weight_bleu[-1])
        scst += scst_dir_suffix(args)
        log_path = pjoin(log_root, '{}_cnnFT_SCST_{}_run_{:02d}'.format(pruned, scst, args.run))
        train_fn_name = 'train_fn_scst'
    args.resume_training = overwrite = os.path.exists(log_path)
    for k, v in list(args.__dict__.items()):
        if v == 'none':
            args.__dict__[k] = None
    kwargs = dict(rnn_layers=1, dropout_rnn_in=0.35, dropout_rnn_out=0.35, rnn_map_loss_scale=1.0, l2_decay=1e-5,
                  clip_gradient_norm=0, max_saves=12, num_logs_per_epoch=100, per_process_gpu_memory_fraction=None,
                  rand_seed=rand_seed, add_image_summaries=True, add_vars_summaries=False, add_grad_summaries=False,
                  log_path=log_path, save_path=pjoin(log_path, 'model'))
    kwargs.update(args.__dict__)
    kwargs.pop('log_root', None)
    if kwargs.get('ema_decay') == 0:            # off: the configuration of a run without the flag
        kwargs.pop('ema_decay')
    if not kwargs.get('label_smoothing'):       # likewise the soft-target flags
        kwargs.pop('label_smoothing', None)
    if not kwargs.get('distill_checkpoints'):
        for k in ('distill_checkpoints', 'distill_weight', 'distill_top_k', 'distill_temperature', 'distill_weights'):
            kwargs.pop(k, None)
    prune.pop_defaults(kwargs)                  # and the pruning flags
    augment.pop_defaults(kwargs)                # and the augmentation flags
    check_supported(kwargs)
    return kwargs, train_fn_name, overwrite


def refuse_unsupported_dtype(train_mode, cnn_dtype):
    """--cnn_dtype f16 runs the frozen CNN only (its backward would need loss scaling: the activation gradients of
    cnn_finetune lie far below the f16 normal range).  Called before anything touches the GPU."""
    if train_mode == 'cnn_finetune' and cnn_dtype == 'f16':
        raise NotImplementedError('--cnn_dtype f16 is forward-only and cannot train the CNN: run --train_mode cnn_finetune '
                                  'with --cnn_dtype bf16 or bf16x3 (decoder / scst runs and infer.py take f16)')


def refuse_bad_ema_decay(ema_decay):
    """--ema_decay outside [0, 1) (1 would freeze the shadow at the initial values).  Called before anything touches the GPU."""
    d = float(ema_decay or 0.0)
    if not 0.0 <= d < 1.0:
        raise ValueError('--ema_decay must be in [0, 1) (0 = off), got {}'.format(ema_decay))


def refuse_bad_prune_options(kw):
    """--prune_*: values out of range, --prune_keep_zeros with --prune_sparsity, schedule flags without --prune_sparsity,
    unknown or never-pruned variable names, an explicit end that is no multiple of --prune_every behind the start.  Called
    before anything touches the GPU."""
    from comic_amd import prune
    prune.refuse_bad_prune_options(kw)


def refuse_bad_augment_options(kw):
    """--cnn_input_augment_crop / _color / _area_min with --cnn_input_augment False, --cnn_input_augment_area_min outside
    (0, 1] or without `area`.  Called before anything touches the GPU."""
    from comic_amd import augment
    augment.refuse_bad_options(kw)


def refuse_bad_soft_options(kw):
    """--label_smoothing / --distill_*: any of them with scst, distillation outside decoder mode, values out of range, and a
    teacher whose configuration (the config.pkl beside its checkpoint) differs from the student's in the token type, the radix
    base, the vocabulary size, the CNN, its input size or the attended feature map.  Called before anything touches the GPU."""
    from comic_amd import distill
    if not any(kw.get(k) for k in distill.FLAGS):
        return
    distill.refuse_bad_soft_options(kw)
    if kw.get('distill_checkpoints') and 'token_type' in kw:
        from types import SimpleNamespace
        distill.check_teachers(SimpleNamespace(**kw))   # (a word / char vocabulary is built later: train_fn checks its size)


def soft_dir_suffixes(args):
    """('_ls0.1', '_kd0.5_k16_t2') for --label_smoothing 0.1 and --distill_weight 0.5 --distill_top_k 16
    --distill_temperature 2 with --distill_checkpoints; '' for a flag at its default."""
    smooth = '_ls%g' % args.label_smoothing if getattr(args, 'label_smoothing', 0.0) else ''
    distil = ''
    if getattr(args, 'distill_checkpoints', ''):
        distil = '_kd%g_k%d_t%g' % (args.distill_weight, args.distill_top_k, args.distill_temperature)
    return smooth, distil


def scst_dir_suffix(args):
    """'_smp' ('_smp_t0.7' when the temperature is not 1) for sampled rollouts and / or '_loo' for the leave-one-out
    baseline; '' for the defaults.  Where the reward is formed changes no name: it changes no result beyond rounding."""
    out = ''
    if getattr(args, 'scst_rollout', 'beam') == 'sample':
        t = float(getattr(args, 'scst_temperature', 1.0))
        out += '_smp' if t == 1.0 else '_smp_t%g' % t
    if getattr(args, 'scst_baseline', 'greedy') == 'mean':
        out += '_loo'
    return out


def refuse_bad_scst_options(kw):
    """--scst_baseline mean, --scst_rollout sample or --scst_reward device with one rollout per image (the one-rollout
    step decodes through another path, which has none of them), --scst_reward device with `char`
    tokens (the device reward works on words) and a temperature that is not finite and > 0.  Called before anything
    touches the GPU."""
    if kw.get('train_mode') != 'scst':
        return
    if kw.get('scst_baseline', 'greedy') == 'mean' and int(kw.get('scst_beam_size', 7)) < 2:
        raise ValueError('--scst_baseline mean needs --scst_beam_size >= 2, got {}'.format(kw.get('scst_beam_size')))
    if kw.get('scst_reward', 'host') == 'device' and kw.get('token_type') == 'char':
        raise ValueError('--scst_reward device needs `word` or `radix` tokens, not `char` (use --scst_reward host)')
    if int(kw.get('scst_beam_size', 7)) < 2 and (kw.get('scst_reward', 'host') == 'device'
                                                 or kw.get('scst_rollout', 'beam') == 'sample'):
        raise ValueError('--scst_rollout sample and --scst_reward device need --scst_beam_size >= 2, got {}'.format(
            kw.get('scst_beam_size')))
    if kw.get('scst_reward', 'host') == 'device' and int(kw.get('scst_beam_size', 7)) > 32:
        raise ValueError('--scst_reward device takes --scst_beam_size <= 32, got {}'.format(kw.get('scst_beam_size')))
    t = float(kw.get('scst_temperature', 1.0))
    if kw.get('scst_rollout', 'beam') == 'sample' and not (t > 0.0 and t < float('inf')):
        raise ValueError('--scst_temperature must be finite and > 0, got {}'.format(kw.get('scst_temperature')))


def check_supported(kw):
    """Options of the reference that this hot path does not implement fail HERE instead of silently training a different
    model.  Refused: --train_mode cnn_finetune with --cnn_dtype f16 (refuse_unsupported_dtype); --scst_baseline mean with
    --scst_beam_size 1 and --scst_reward device with `char` tokens (refuse_bad_scst_options).  --clip_gradient_norm
    (model_base.py:394-401) is per-variable tf.clip_by_norm in front of the optimiser (optim.GradClip), --rnn_name
    LN_LSTM / GRU (model_base.py:622-629) run on the per-step launch chain."""
    refuse_unsupported_dtype(kw.get('train_mode'), kw.get('cnn_dtype'))
    refuse_bad_ema_decay(kw.get('ema_decay'))
    refuse_bad_scst_options(kw)
    refuse_bad_soft_options(kw)
    refuse_bad_prune_options(kw)
    refuse_bad_augment_options(kw)
    bad = []
    # --initialiser: `he` / `none` select TensorFlow's default initialiser in the reference (model_base.py:823-831:
    # every value but `xavier` returns None), which for these float variables is glorot_uniform == Xavier-uniform
    # [TF-1.9 get_variable default]: all three choices build the same model, here too.
    if bad:
        raise NotImplementedError('not implemented on the MI355X hot path: ' + '; '.join(bad))


def main(argv=None):
    args = create_parser().parse_args(argv)
    refuse_unsupported_dtype(args.train_mode, args.cnn_dtype)
    refuse_bad_ema_decay(args.ema_decay)
    refuse_bad_scst_options(vars(args))
    refuse_bad_soft_options(vars(args))
    refuse_bad_prune_options(vars(args))
    refuse_bad_augment_options(vars(args))
    import torch
    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(args.gpu).split(',')[0] if world == 1 else '0'))
    # COMIC_DIST_BACKEND=gloo: data-parallel rehearsal on fewer GPUs than ranks (the ranks share the visible devices)
    backend = os.environ.get('COMIC_DIST_BACKEND', 'nccl')
    if backend != 'nccl':
        local_rank %= max(1, torch.cuda.device_count())
        if int(os.environ.get('LOCAL_WORLD_SIZE', str(world))) > torch.cuda.device_count():
            # ranks sharing a GPU cannot both keep a persistent loop's workgroups resident: per-step launches (bench.py)
            os.environ.setdefault('COMIC_PERSIST', '0')
    torch.cuda.set_device(local_rank)
    device = 'cuda:%d' % local_rank
    if world > 1:
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device(device))
        else:
            dist.init_process_group(backend)
    # every rank decides "new run or resume" from the SAME state of the experiments directory: the decision is taken
    # (build_kwargs looks at log_path) before any rank may create it (try_to_train, behind this barrier)
    kwargs, train_fn_name, overwrite = build_kwargs(args)
    if world > 1:
        dist.barrier()
    from comic_amd import train_fn as train
    from comic_amd.trainer import DataParallel
    dp = None
    if world > 1:
        dp = DataParallel(dist)
        # rand_seed stays the SAME on every rank: it seeds the parameter initialisers and the common shuffle; the
        # input managers shard the shuffled list by rank (config.dp_world / dp_rank)
        kwargs['dp_world'], kwargs['dp_rank'] = dp.world, dp.rank
    fn = getattr(train, train_fn_name)
    train.try_to_train(train_fn=lambda cfg: fn(cfg, device=device, dp=dp), try_block=True, overwrite=overwrite, **kwargs)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
