"""Gradual magnitude pruning of the decoder's weight matrices (`--prune_sparsity`; Zhu & Gupta 2017, "To prune, or not to
prune").  Host side: the flags and their refusals, the cubic schedule, the groups and their targets, and `PruneMask` -- the
device mask of a flat parameter buffer with its mask events (csrc/prune.hip through comic_prune_select).  The optimisers
(optim.AdamTF / MomentumTF, `prune=`) launch the masked update and run the events; checkpoints carry the mask words under
MASK_KEY."""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L

# the decoder variables with two dimensions (DecoderSpec.param_shapes(), where present); biases, LayerNorm vectors and tau
# are never pruned
PRUNABLE = ('W_init', 'K', 'K_c', 'W_m', 'W_v', 'W_q', 'W_a', 'W_o', 'emb')
SCOPES = ('layer', 'global')
MASK_KEY = 'optimise/caption/prune_mask'
FLAGS = ('prune_sparsity', 'prune_start_step', 'prune_end_step', 'prune_every', 'prune_scope', 'prune_variables',
         'prune_keep_zeros')
DEFAULTS = dict(prune_sparsity=0.0, prune_start_step=-1, prune_end_step=-1, prune_every=100, prune_scope='layer',
                prune_variables='', prune_keep_zeros=False)


def prune_sparsity_at(t, s_f, t0, t1):
    """The scheduled sparsity after optimiser update t: 0 before t0, s_f after t1, between them
    s_f * (1 - (1 - (t - t0) / (t1 - t0))^3) (float64)."""
    if t < t0:
        return 0.0
    if t >= t1:
        return float(s_f)
    return float(s_f) * (1.0 - (1.0 - (t - t0) / float(t1 - t0)) ** 3)


def target_count(s_t, n):
    """k = floor(s_t * n) in float64: the pruned elements of a group of n real elements at sparsity s_t."""
    return int(math.floor(np.float64(s_t) * np.float64(n)))


def is_event(t, t0, t1, every):
    return t0 <= t <= t1 and (t - t0) % every == 0


def active(kw):
    """Whether a configuration (dict or object) prunes or keeps zeros at all."""
    get = kw.get if isinstance(kw, dict) else lambda k, d=None: getattr(kw, k, d)
    return bool(get('prune_sparsity', 0) or get('prune_keep_zeros', False))


def parse_variables(text):
    """'W_m,K' -> ('W_m', 'K'); '' / None -> None (the default: every prunable variable of the model).  Unknown names and
    names of variables that are never pruned are refused."""
    if not text:
        return None
    names = tuple(s.strip() for s in (text.split(',') if isinstance(text, str) else text) if str(s).strip())
    for n in names:
        if n in PRUNABLE:
            continue
        if n in L.PARAM_NAMES and n != 'status' or n.startswith('cln_'):
            raise ValueError('--prune_variables: `{}` is never pruned (biases, LayerNorm vectors and tau stay dense); '
                             'prunable: {}'.format(n, ', '.join(PRUNABLE)))
        raise ValueError('--prune_variables: unknown variable `{}`; prunable: {}'.format(n, ', '.join(PRUNABLE)))
    if len(set(names)) != len(names):
        raise ValueError('--prune_variables names a variable twice: {}'.format(text))
    return names


def refuse_bad_prune_options(kw):
    """--prune_*: values out of range, --prune_keep_zeros together with --prune_sparsity, schedule flags without
    --prune_sparsity, unknown or non-prunable variable names, and an explicit start / end whose distance is no multiple of
    --prune_every.  Called before anything touches the GPU."""
    g = lambda k: DEFAULTS[k] if kw.get(k) is None else kw.get(k)
    s = float(g('prune_sparsity'))
    keep = bool(g('prune_keep_zeros'))
    if not (0.0 <= s < 1.0):                      # (NaN fails both comparisons)
        raise ValueError('--prune_sparsity must be in (0, 1) (0 = off), got {}'.format(kw.get('prune_sparsity')))
    if keep and s > 0:
        raise ValueError('--prune_keep_zeros freezes the zeros of the loaded checkpoint and runs no schedule: it cannot be '
                         'combined with --prune_sparsity')
    parse_variables(g('prune_variables'))
    scope = g('prune_scope')
    if scope not in SCOPES:
        raise ValueError('--prune_scope must be `layer` or `global`, got {}'.format(scope))
    t0, t1, dt = int(g('prune_start_step')), int(g('prune_end_step')), int(g('prune_every'))
    if s == 0:
        given = [k for k in ('prune_start_step', 'prune_end_step', 'prune_every', 'prune_scope') if g(k) != DEFAULTS[k]]
        if not keep and g('prune_variables'):
            given.append('prune_variables')
        if given:
            raise ValueError('--{} without --prune_sparsity: there is no schedule to run'.format(given[0]))
        return
    if dt < 1:
        raise ValueError('--prune_every must be >= 1, got {}'.format(dt))
    if t0 < -1 or t1 < -1:
        raise ValueError('--prune_start_step / --prune_end_step must be >= 0, got {} / {}'.format(t0, t1))
    if t0 >= 0 and t1 >= 0:
        if t1 <= t0:
            raise ValueError('--prune_end_step {} must be above --prune_start_step {}'.format(t1, t0))
        if (t1 - t0) % dt:
            raise ValueError('--prune_end_step - --prune_start_step = {} is no multiple of --prune_every {}'.format(t1 - t0, dt))


def dir_suffix(args):
    """'_pr0.8' for --prune_sparsity 0.8 (`layer` scope), '_pr0.8g' for `global`; '' when off and for --prune_keep_zeros."""
    s = float(getattr(args, 'prune_sparsity', 0) or 0)
    if not s:
        return ''
    return '_pr%g%s' % (s, 'g' if getattr(args, 'prune_scope', 'layer') == 'global' else '')


def pop_defaults(kwargs):
    """A configuration without pruning holds none of the keys (as `ema_decay`)."""
    if not active(kwargs):
        for k in FLAGS:
            kwargs.pop(k, None)


class PruneSpec:
    """The resolved options of one run: sparsity s_f, events at t0, t0 + every, ..., t1, `scope`, the variables, or
    keep_zeros (a frozen mask `w != 0`, no schedule)."""

    def __init__(self, sparsity=0.0, start=0, end=0, every=100, scope='layer', variables=None, keep_zeros=False):
        self.sparsity, self.start, self.end, self.every = float(sparsity), int(start), int(end), int(every)
        self.scope, self.keep_zeros = scope, bool(keep_zeros)
        self.variables = tuple(variables) if variables is not None else None
        if self.keep_zeros:
            if self.sparsity:
                raise ValueError('keep_zeros runs no schedule: sparsity must be 0')
            return
        if not 0.0 < self.sparsity < 1.0:
            raise ValueError('sparsity must be in (0, 1): %r' % (sparsity,))
        if scope not in SCOPES:
            raise ValueError('scope must be `layer` or `global`: %r' % (scope,))
        if self.every < 1 or self.start < 0 or self.end <= self.start or (self.end - self.start) % self.every:
            raise ValueError('events every %d updates from %d to %d: the distance must be a positive multiple'
                             % (self.every, self.start, self.end))

    @classmethod
    def from_config(cls, c, max_step):
        """None when the configuration does not prune.  Defaults: start and end at 10 % and 60 % of max_step, a defaulted
        end moved down so that end - start is a multiple of `every`."""
        if not active(c):
            return None
        kw = {k: getattr(c, k, DEFAULTS[k]) for k in FLAGS}
        refuse_bad_prune_options(kw)
        g = lambda k: DEFAULTS[k] if kw[k] is None else kw[k]
        names = parse_variables(g('prune_variables'))
        if g('prune_keep_zeros'):
            return cls(keep_zeros=True, variables=names)
        t0, t1, dt = int(g('prune_start_step')), int(g('prune_end_step')), int(g('prune_every'))
        if t0 < 0:
            t0 = int(0.1 * max_step)
        if t1 < 0:
            t1 = int(0.6 * max_step)
            t1 = t0 + (t1 - t0) // dt * dt
            if t1 <= t0:
                raise ValueError('--prune_every {} leaves no event between step {} and 60 % of max_step {}: pass '
                                 '--prune_end_step'.format(dt, t0, max_step))
        return cls(float(g('prune_sparsity')), t0, t1, dt, g('prune_scope'), names)

    def sparsity_at(self, t):
        return prune_sparsity_at(t, self.sparsity, self.start, self.end)

    def event_at(self, t):
        return not self.keep_zeros and is_event(t, self.start, self.end, self.every)


def segments_of(shapes, offsets, variables=None, scope='layer'):
    """The segment table of a flat buffer: [(name, first element, elements, group)] ascending by first element, one group per
    variable (`layer`) or one for all (`global`); `variables` None: every prunable variable the shapes hold."""
    if variables is None:
        variables = [k for k in shapes if k in PRUNABLE]
    for k in variables:
        if k not in shapes:
            raise ValueError('--prune_variables: this model has no variable `{}` (it has {})'.format(
                k, ', '.join(n for n in shapes if n in PRUNABLE)))
        if len(shapes[k]) != 2:
            raise ValueError('only variables with two dimensions are pruned: `{}` has shape {}'.format(k, shapes[k]))
    rows = sorted((offsets[k], k) for k in variables)
    if not rows:
        raise ValueError('nothing to prune: the model has none of {}'.format(', '.join(PRUNABLE)))
    return [(k, off, int(np.prod(shapes[k])), i if scope == 'layer' else 0) for i, (off, k) in enumerate(rows)]


class PruneMask:
    """The mask of one FlatParams buffer on its device (uint32 words, bit i % 32 of word i / 32 = element i is live) and the
    mask events of a PruneSpec on it."""

    def __init__(self, params, spec):
        import torch
        self.torch, self.lib, self.spec, self.params = torch, L.load(), spec, params
        self.segments = segments_of(params.shapes, params.offsets, spec.variables, spec.scope)
        self.n_groups = 1 + max(s[3] for s in self.segments)
        self.group_sizes = [sum(s[2] for s in self.segments if s[3] == g) for g in range(self.n_groups)]
        self.n_total = int(params.numel)
        dev = params.device
        self.words = torch.full(((self.n_total + 31) // 32,), -1, dtype=torch.int32, device=dev)     # all live
        self.table = torch.from_numpy(np.asarray([s[1:] for s in self.segments], np.int64)).to(dev)
        ws = int(self.lib.comic_prune_workspace_bytes(self.n_total, len(self.segments), self.n_groups))
        if ws < 0:
            raise ValueError('comic_prune_workspace_bytes refused the table')
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        self.targets = torch.zeros(self.n_groups, dtype=torch.int64, device=dev)
        self.events = 0

    def targets_at(self, s_t):
        return [target_count(s_t, n) for n in self.group_sizes]

    def select(self, targets, m, v, shadow=None):
        """One mask event with the per-group targets (pruned elements afterwards), on the current stream."""
        self.targets.copy_(self.torch.tensor([int(k) for k in targets], dtype=self.torch.int64), non_blocking=False)
        L.check(self.lib.comic_prune_select(self.params.data.data_ptr(), self.words.data_ptr(), self.n_total,
                                            self.table.data_ptr(), len(self.segments), self.targets.data_ptr(),
                                            self.n_groups, m.data.data_ptr(), v.data.data_ptr(),
                                            shadow.data.data_ptr() if shadow is not None else None,
                                            self.workspace.data_ptr(), self.workspace.numel(), L.stream_ptr()), 'prune_select')
        self.events += 1

    def event(self, t, m, v, shadow=None):
        self.select(self.targets_at(self.spec.sparsity_at(t)), m, v, shadow)

    def mask_buffer(self, buf, lo=0, hi=None):
        """+0.0f at the pruned elements [lo, hi) of a buffer laid out like the parameters."""
        hi = self.n_total if hi is None else hi
        L.check(self.lib.comic_prune_mask_buffer(buf.data.data_ptr() + 4 * lo, self.words.data_ptr(), lo, hi - lo,
                                                 L.stream_ptr()), 'prune_mask_buffer')

    def from_zeros(self, *also):
        """The mask of --prune_keep_zeros: `w != 0` on the prunable variables as they are now; `also` (slots, shadow) get
        +0.0f where the mask is clear, and so do the variables (a loaded -0.0 becomes +0.0)."""
        L.check(self.lib.comic_prune_mask_from_zeros(self.params.data.data_ptr(), self.words.data_ptr(), self.n_total,
                                                     self.table.data_ptr(), len(self.segments), L.stream_ptr()),
                'prune_mask_from_zeros')
        for b in (self.params,) + tuple(b for b in also if b is not None):
            self.mask_buffer(b)

    def to_numpy(self):
        return self.words.cpu().numpy().view(np.uint32).copy()

    def load(self, words):
        w = np.ascontiguousarray(np.asarray(words).reshape(-1)).astype(np.uint32, copy=False)
        if w.shape[0] != self.words.shape[0]:
            raise ValueError('prune mask of %d words for a buffer of %d' % (w.shape[0], self.words.shape[0]))
        self.words.copy_(self.torch.from_numpy(w.view(np.int32)))

    def pruned_counts(self):
        """{variable: pruned elements} from the device mask (synchronises)."""
        return {k: n - c for k, (c, n) in live_counts(self.to_numpy(), self.segments).items()}


def live_counts(words, segments):
    """{variable: (live elements, elements)} of a host mask."""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype='<u4').view(np.uint8), bitorder='little')
    return {k: (int(bits[off:off + n].sum()), n) for k, off, n, _ in segments}


def size_block(step, s_t, counts, total_nonzero, total):
    """The block a checkpoint save appends to model_size.txt while pruning is on: counts = {variable: (non-zero, size)};
    s_t None: --prune_keep_zeros (no schedule)."""
    lines = ['Pruning ~ step {} ~ {}'.format(int(step), 'zeros of the loaded checkpoint kept' if s_t is None else
                                             'scheduled sparsity {:.6f}'.format(float(s_t)))]
    lines += ['{} : {:,d} / {:,d} non-zero'.format(k, nz, n) for k, (nz, n) in counts.items()]
    lines.append('Scope `Model/decoder/rnn_decoder` : {:,d} / {:,d} non-zero parameters'.format(int(total_nonzero), int(total)))
    return '\r\n' + '\r\n'.join(lines) + '\r\n\r\n'
