"""Soft-target XE training behind the command line: the checks of --label_smoothing / --distill_* that need no GPU, and the
teacher decoder(s) of a distilled run (decoder.SoftTargets, Decoder.teacher_targets, EnsembleDecoder.teacher_targets).

A teacher is a `model_compact-N` / `model_ema-N` checkpoint with its run's `config.pkl` beside it.  Distillation runs in
--train_mode decoder, where the CNN is frozen: student and teachers read ONE feature map, so a teacher must agree with the
student in everything the features and the token ids depend on (TEACHER_FIELDS and the vocabulary size)."""
import os

from . import checkpoint as ckpt
from . import configuration as conf
from . import decoder as cdec

TEACHER_FIELDS = ('token_type', 'radix_base', 'cnn_name', 'cnn_input_size', 'cnn_fm_attention')
FLAGS = ('label_smoothing', 'distill_checkpoints', 'distill_weight', 'distill_top_k', 'distill_temperature', 'distill_weights')


def checkpoint_list(value):
    """--distill_checkpoints p1[,p2...] (or a list) -> the paths"""
    if not value:
        return []
    return [p.strip() for p in value.split(',') if p.strip()] if isinstance(value, str) else list(value)


def weight_list(value, n):
    """--distill_weights w1,... -> n floats (checked by decoder.check_ensemble later), or None"""
    if value in (None, ''):
        return None
    w = [float(x) for x in value.split(',')] if isinstance(value, str) else [float(x) for x in value]
    if len(w) != n:
        raise ValueError('--distill_weights has %d entries for %d --distill_checkpoints' % (len(w), n))
    if any(not x >= 0.0 for x in w) or abs(sum(w) - 1.0) > 1e-6:
        raise ValueError('--distill_weights must be >= 0 and sum to 1, got %r' % (w,))
    return w


def refuse_bad_soft_options(kw):
    """Every refusal of the soft-target flags that needs nothing but the flags: any of them with scst, distillation
    outside decoder mode, values out of range, a weight without a teacher.  Called before anything touches the GPU."""
    eps = float(kw.get('label_smoothing', 0.0) or 0.0)
    paths = checkpoint_list(kw.get('distill_checkpoints'))
    lam = float(kw.get('distill_weight', 0.0) or 0.0)
    given = eps != 0.0 or bool(paths) or lam != 0.0 or kw.get('distill_weights') not in (None, '')
    if not given:
        return
    mode = kw.get('train_mode')
    if mode == 'scst':
        raise ValueError('--label_smoothing / --distill_* are XE training: not available with --train_mode scst')
    if (paths or lam != 0.0 or kw.get('distill_weights') not in (None, '')) and mode != 'decoder':
        raise ValueError('--distill_* needs --train_mode decoder (the frozen CNN gives student and teachers one feature '
                         'map), got %s' % mode)
    if lam != 0.0 and not paths:
        raise ValueError('--distill_weight %g without --distill_checkpoints' % lam)
    if paths and lam == 0.0:
        raise ValueError('--distill_checkpoints needs --distill_weight in (0, 1]')
    if not 1 <= len(paths) <= 8 and paths:
        raise ValueError('--distill_checkpoints takes 1 to 8 checkpoints, got %d' % len(paths))
    k, tau = kw.get('distill_top_k'), kw.get('distill_temperature')
    cdec.SoftTargets(eps, lam, 16 if k is None else int(k), 1.0 if tau is None else float(tau))
    weight_list(kw.get('distill_weights'), len(paths))


def teacher_config(path):
    """The configuration of a teacher checkpoint: the config.pkl beside it."""
    f = os.path.join(os.path.dirname(os.path.abspath(path)), 'config.pkl')
    if not os.path.isfile(f):
        raise ValueError('--distill_checkpoints: no config.pkl beside %s' % path)
    return conf.load_config(f)


def vocabulary_size(c):
    return c.radix_base + 2 if c.token_type == 'radix' else len(c.itow)


def check_teacher_config(student, teacher, path):
    """A teacher that differs from the student in the token type, the radix base, the vocabulary size, the CNN, its input
    size or the attended feature map is refused (ValueError)."""
    def norm(f, v):
        if f == 'cnn_input_size' and v is not None:
            return [int(x) for x in (v.split(',') if isinstance(v, str) else v)]
        return v
    for f in TEACHER_FIELDS:
        a, b = norm(f, getattr(student, f, None)), norm(f, getattr(teacher, f, None))
        if f == 'radix_base' and getattr(student, 'token_type', None) != 'radix':
            continue
        if a != b:
            raise ValueError('--distill_checkpoints: teacher %s differs from the student in %s: %r against %r' % (path, f, b, a))
    known = student.token_type == 'radix' or hasattr(student, 'itow')      # (the command line knows no word list yet)
    if known and vocabulary_size(student) != vocabulary_size(teacher):
        raise ValueError('--distill_checkpoints: teacher %s differs from the student in the vocabulary size: %d against %d'
                         % (path, vocabulary_size(teacher), vocabulary_size(student)))
    if getattr(student, 'legacy', False) or getattr(teacher, 'legacy', False):
        raise ValueError('--distill_checkpoints: legacy models (an encoder head of their own) do not distil')


def check_teachers(c):
    """The teachers' configurations against the student's, from the files alone.  -> [(path, teacher configuration)]"""
    out = []
    for path in checkpoint_list(getattr(c, 'distill_checkpoints', None)):
        if not (os.path.isfile(path) or os.path.isfile(path + '.npz') or os.path.isfile(path + '.index')):
            raise ValueError('--distill_checkpoints: checkpoint not found: %s' % path)
        tc = teacher_config(path)
        check_teacher_config(c, tc, path)
        out.append((path, tc))
    return out


def load_teachers(c, student_spec, device):
    """The teacher of a distilled run: an EnsembleDecoder over the checkpoints' decoders (each with the geometry of its own
    configuration, on the student's feature-map and embedding sizes), weighted by --distill_weights.  None without
    --distill_checkpoints."""
    members = check_teachers(c)
    if not members:
        return None
    decoders = []
    for path, tc in members:
        spec = cdec.DecoderSpec.from_config(tc, (student_spec.M, student_spec.C), student_spec.Cg)
        file = path if os.path.isfile(path) or os.path.isfile(path + '.index') else path + '.npz'
        _, params, _ = ckpt.restore(file, [], spec)
        if params is None:
            raise ValueError('--distill_checkpoints: %s holds no decoder variables' % path)
        decoders.append(cdec.Decoder(spec, params, device))
        print('INFO: Distillation teacher restored from checkpoint: {}'.format(path))
    return cdec.EnsembleDecoder(decoders, weight_list(getattr(c, 'distill_weights', None), len(decoders)))
