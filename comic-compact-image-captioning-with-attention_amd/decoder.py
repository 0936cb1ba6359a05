"""Host side of the attention-LSTM decoder: parameter storage, input processing and the
calls into the native executors (`comic_decoder_train_step / _greedy / _beam`).

Counterpart of the decoder half of `ModelBase` (reference src/model_base.py:109-314,
:501-757) and of `common/ops_rnn.py`'s three dynamic-decode builders.  All arithmetic is in
the HIP library; this module only prepares integer/mask tables on the host (the reference
does the same work in `_process_inputs`, model_base.py:501-528) and post-processes ids.

Parameters live in ONE flat fp32 device buffer (views per variable) so that the optimiser
is a single fused kernel and the data-parallel gradient exchange is a single all-reduce.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L
from .ops import number_to_base

# TF variable names (scope Model/decoder/rnn_decoder/), SURVEY Appendix C
# TensorFlow variable names under `Model/decoder/rnn_decoder/` (checkpoint.decoder_var_names composes them; derived from
# the reference's scopes by oracle/ref_var_names.py and pinned by tests/golden/ref_var_names.json):
#   * created when the graph is CONSTRUCTED (model_base.py:147-176): memory / value layers, output projection, embedding
#     map, the rnn-init projection;
#   * STEP_VARS are created at the first decoder step, i.e. inside dynamic_decode's 'decoder' scope and the attention
#     wrapper's own layer scope (ops_rnn.py:543-562, :735);
#   * CELL_VARS follow the cell's FIRST call: 'rnn_init_input/' with rnn_init_method='first_input' (model_base.py:677-686),
#     the step scope with 'project_hidden'.
STEP_SCOPE = 'decoder/multi_head_attention_wrapper_v3/'
TF_NAMES = {
    'W_init': {'first_input': 'rnn_init_input/projection/weight', 'project_hidden': 'rnn_initial_state/weight'},
    'K': 'basic_lstm_cell/kernel', 'b': 'basic_lstm_cell/bias',
    'W_m': 'memory_layer/kernel', 'W_v': 'value_layer/kernel',
    'W_q': 'multi_add_attention/query_layer/kernel', 'v': 'multi_add_attention/attention_v',
    'ln_g': 'multi_add_attention/LN_tanh/gamma', 'ln_b': 'multi_add_attention/LN_tanh/beta',
    'tau': 'softmax_temperature', 'W_a': 'a_layer/kernel',
    'W_o': 'output_projection/kernel', 'b_o': 'output_projection/bias', 'emb': 'embedding_map',
    # --rnn_name GRU: tf.contrib.rnn.GRUCell's candidate pair (its gates pair takes K / b)
    'K_c': 'gru_cell/candidate/kernel', 'b_c': 'gru_cell/candidate/bias',
}
STEP_VARS = ('W_q', 'v', 'ln_g', 'ln_b', 'tau', 'W_a')
# per cell: TF scope of the cell's variables and the names of K / b inside it (model_base.py:606-632)
CELL_SCOPES = {'LSTM': ('basic_lstm_cell', 'kernel', 'bias'), 'LN_LSTM': ('layer_norm_basic_lstm_cell', 'kernel', None),
               'GRU': ('gru_cell', 'gates/kernel', 'gates/bias')}
# --rnn_name LN_LSTM: LayerNormBasicLSTMCell's five layer_norm scopes, in the order of comic_decoder_params::cell_ln
LN_LSTM_NORMS = (('i', 'input'), ('j', 'transform'), ('f', 'forget'), ('o', 'output'), ('c', 'state'))
for _k, _scope in LN_LSTM_NORMS:
    TF_NAMES['cln_%sg' % _k] = 'layer_norm_basic_lstm_cell/%s/gamma' % _scope
    TF_NAMES['cln_%sb' % _k] = 'layer_norm_basic_lstm_cell/%s/beta' % _scope
CELL_VARS = ('K', 'b', 'K_c', 'b_c') + tuple('cln_%s%s' % (k, s) for k, _ in LN_LSTM_NORMS for s in 'gb')


@dataclass
class DecoderSpec:
    """Static decoder geometry derived from a reference `Config` (src/train.py:29-162)."""
    D: int = 512
    E: int = 256
    V: int = 258
    C: int = 2048
    Cg: int = 2048
    H: int = 8
    M: int = 25
    fm_projection: str | None = 'tied'
    method: str = 'add_LN'
    prob: str = 'softmax'
    context_layer: bool = False
    init_method: str = 'first_input'
    token_type: str = 'radix'
    start_id: int = 256
    end_id: int = 257
    dropout_rnn_in: float = 0.35
    dropout_rnn_out: float = 0.35
    attn_keep_prob: float = 0.9
    map_loss_scale: float = 1.0
    l2_decay: float = 1e-5
    recurrent_dropout: bool = False      # DropoutWrapper(variational_recurrent=True): ONE input / output mask row
                                         # for all batch rows and time steps of a run [TF-1.9: noise shape [1, size]]
    rnn_name: str = 'LSTM'               # 'LSTM' | 'LN_LSTM' | 'GRU' (model_base.py:606-632); the persistent / fused /
                                         # streaming kernels are BasicLSTMCell's, the other two run per-step launches

    @property
    def A(self):                     # model_base.py:611-615
        return self.C if (self.fm_projection is None and not self.context_layer) else self.D

    @property
    def Cv(self):
        return self.C if self.fm_projection is None else self.D

    @classmethod
    def from_config(cls, c, fm_shape, im_embed_size):
        """c: reference-style Config (token_type, radix_base, rnn_size, ... itow/wtoi)."""
        if c.rnn_name not in L.CELLS:
            raise ValueError('Only `LSTM`, `LN_LSTM` and `GRU` are accepted.')      # model_base.py:631
        if c.attn_alignment_method not in ('add_LN', 'dot'):
            raise ValueError('Invalid alignment method.')          # model_base.py:133-138
        if c.attn_probability_fn not in ('softmax', 'sigmoid'):
            raise ValueError('Invalid alignment method.')
        if c.token_type == 'radix':
            V, start, end = c.radix_base + 2, c.radix_base, c.radix_base + 1     # model_base.py:42-43,701-703
        else:
            V, start, end = len(c.itow), c.wtoi['<GO>'], c.wtoi['<EOS>']
        return cls(D=c.rnn_size, E=c.rnn_word_size, V=V, C=fm_shape[-1], Cg=im_embed_size, H=c.attn_num_heads,
                   M=fm_shape[-2], fm_projection=c.cnn_fm_projection, method=c.attn_alignment_method,
                   prob=c.attn_probability_fn, context_layer=bool(c.attn_context_layer),
                   init_method=c.rnn_init_method, token_type=c.token_type, start_id=start, end_id=end,
                   dropout_rnn_in=getattr(c, 'dropout_rnn_in', 0.35), dropout_rnn_out=getattr(c, 'dropout_rnn_out', 0.35),
                   attn_keep_prob=c.attn_keep_prob, map_loss_scale=getattr(c, 'rnn_map_loss_scale', 1.0),
                   l2_decay=getattr(c, 'l2_decay', 1e-5), recurrent_dropout=bool(getattr(c, 'rnn_recurr_dropout', False)),
                   rnn_name=c.rnn_name)

    def param_shapes(self):
        D, E, A, V, C_, Cg = self.D, self.E, self.A, self.V, self.C, self.Cg
        s = {}
        s['W_init'] = (Cg, E + A) if self.init_method == 'first_input' else (Cg, D)
        if self.rnn_name == 'GRU':
            s['K'] = (E + A + D, 2 * D); s['b'] = (2 * D,)
            s['K_c'] = (E + A + D, D); s['b_c'] = (D,)
        elif self.rnn_name == 'LN_LSTM':       # no bias; the ten LayerNorm vectors are consecutive views (cell_ln)
            s['K'] = (E + A + D, 4 * D)
            for k, _ in LN_LSTM_NORMS:
                s['cln_%sg' % k] = (D,); s['cln_%sb' % k] = (D,)
        else:
            s['K'] = (E + A + D, 4 * D)
            s['b'] = (4 * D,)
        s['W_m'] = (C_, D)
        if self.fm_projection == 'independent':
            s['W_v'] = (C_, D)
        s['W_q'] = (D, D)
        if self.method == 'add_LN':
            s['v'] = (D,); s['ln_g'] = (D,); s['ln_b'] = (D,); s['tau'] = ()
        if self.context_layer:
            s['W_a'] = (self.Cv, D)
        s['W_o'] = (D, V)
        s['b_o'] = (V,)
        s['emb'] = (V, E)
        return s

    def desc(self, training):
        d = L.DecoderDesc()
        d.D, d.E, d.A, d.V, d.C, d.Cg, d.H, d.M, d.Cv = (self.D, self.E, self.A, self.V, self.C, self.Cg, self.H,
                                                       self.M, self.Cv)
        d.fm_projection = {None: 0, 'independent': 1, 'tied': 2}[self.fm_projection]
        d.method = {'add_LN': 0, 'dot': 1}[self.method]
        d.prob = {'softmax': 0, 'sigmoid': 1}[self.prob]
        d.context_layer = int(self.context_layer)
        d.init_method = {'first_input': 0, 'project_hidden': 1}[self.init_method]
        d.start_id, d.end_id = self.start_id, self.end_id
        d.keep_in = 1.0 - self.dropout_rnn_in if training else 1.0
        d.keep_out = 1.0 - self.dropout_rnn_out if training else 1.0
        d.keep_alpha = self.attn_keep_prob if training else 1.0
        d.map_loss_scale = self.map_loss_scale
        d.flags = L.decoder_flags_from_env()
        d.cell = L.CELLS[self.rnn_name]
        return d


def xavier_uniform(rng, shape):
    """slim.xavier_initializer() [TF-1.9] (model_base.py:823-831)."""
    if len(shape) > 1:
        fi, fo = shape[-2], shape[-1]
    else:
        fi = fo = shape[-1]
    lim = math.sqrt(6.0 / (fi + fo))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def init_params(spec: DecoderSpec, seed=0):
    rng = np.random.default_rng(seed)
    p = {}
    for k, shp in spec.param_shapes().items():
        if k == 'b' and spec.rnn_name == 'GRU':
            p[k] = np.ones(shp, np.float32)                        # [TF-1.9] GRUCell: gates bias starts at 1.0
        elif k in ('b', 'b_o', 'ln_b', 'b_c') or (k.startswith('cln_') and k.endswith('b')):
            p[k] = np.zeros(shp, np.float32)
        elif k == 'ln_g' or (k.startswith('cln_') and k.endswith('g')):
            p[k] = np.ones(shp, np.float32)
        elif k == 'tau':
            p[k] = np.array(5.0, np.float32)                       # ops_rnn.py:559
        else:
            p[k] = xavier_uniform(rng, shp)
    return p


class FlatParams:
    """One flat fp32 device buffer with named views (+ identical layouts for grads/Adam slots)."""
    ALIGN = 64      # floats: keeps every view 256-byte aligned (16-byte vector loads in the GEMM)

    def __init__(self, shapes: dict, device='cuda:0', status_tail=False):
        import torch
        self.torch = torch
        self.shapes = dict(shapes)
        self.offsets = {}
        off = 0
        for k, shp in shapes.items():
            self.offsets[k] = off
            n = int(np.prod(shp)) if len(shp) else 1
            off += (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = off
        self.device = device
        # status_tail: one aligned block behind the variables whose first float is the buffer's status word
        # (comic_decoder_params::status: voided-step flag of a gradient buffer, sticky count of a parameter buffer)
        self.tail = self.ALIGN if status_tail else 0
        self.data = torch.zeros(off + self.tail, dtype=torch.float32, device=device)

    def like(self):
        o = FlatParams.__new__(FlatParams)
        o.torch, o.shapes, o.offsets, o.numel, o.device = self.torch, self.shapes, self.offsets, self.numel, self.device
        o.tail = self.tail
        o.data = self.torch.zeros(self.numel + self.tail, dtype=self.torch.float32, device=self.device)
        return o

    @property
    def status(self):
        """The status word (a 1-element view) or None."""
        return self.data[self.numel:self.numel + 1] if self.tail else None

    @property
    def flat(self):
        """The variables without the status tail (what checkpoints hold)."""
        return self.data[:self.numel]

    def view(self, k):
        shp = self.shapes[k]
        n = int(np.prod(shp)) if len(shp) else 1
        return self.data[self.offsets[k]:self.offsets[k] + n].view(*shp) if len(shp) else \
            self.data[self.offsets[k]:self.offsets[k] + 1]

    def load(self, values: dict):
        for k in self.shapes:
            v = self.torch.from_numpy(np.ascontiguousarray(values[k], np.float32).reshape(-1))
            self.view(k).reshape(-1).copy_(v)

    def to_numpy(self):
        return {k: self.view(k).detach().cpu().numpy().reshape(self.shapes[k]) for k in self.shapes}

    def table(self):
        t = L.DecoderParams()
        base = self.data.data_ptr()
        for k in L.PARAM_NAMES:
            setattr(t, k, base + 4 * self.offsets[k] if k in self.offsets else None)
        t.status = base + 4 * self.numel if self.tail else None
        if 'cln_ig' in self.offsets:          # LN_LSTM: the ten vectors are consecutive views, ALIGN-padded (= the C stride)
            t.cell_ln = base + 4 * self.offsets['cln_ig']
        return t

    def n_params(self):
        return int(sum(int(np.prod(s)) if len(s) else 1 for s in self.shapes.values()))


class _Keyed:
    """Equality and hash of an immutable option class, from its key()."""

    def __eq__(self, other):
        return type(other) is type(self) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())


class BeamConstraints(_Keyed):
    """What a beam may emit (comic_beam_constraints; extends rnn_decoder_beam_search, ops_rnn.py:49-112), in TOKENS:
    min_length: no <EOS> before that many tokens; no_repeat_ngram = n: no n-gram twice (0: off), with windows that start at
    multiples of ngram_stride (n % ngram_stride == 0; the radix word length makes the windows whole words); suppress: up to
    32 token ids that are never emitted.  Immutable and hashable: decode contexts are keyed by it."""
    MAX_SUPPRESS = 32
    MAX_WORDS = 2048                 # mask words of a row: V <= 65 536

    def __init__(self, min_length=0, no_repeat_ngram=0, ngram_stride=1, suppress=()):
        self.min_length, self.no_repeat_ngram, self.ngram_stride = int(min_length), int(no_repeat_ngram), int(ngram_stride)
        self.suppress = tuple(int(x) for x in suppress)

    def key(self):
        return (self.min_length, self.no_repeat_ngram, self.ngram_stride, self.suppress)

    def __repr__(self):
        return 'BeamConstraints(min_length=%d, no_repeat_ngram=%d, ngram_stride=%d, suppress=%r)' % self.key()

    @property
    def active(self):
        return bool(self.min_length > 0 or self.no_repeat_ngram > 0 or self.suppress)

    def check(self, spec, beam, max_steps):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field."""
        V = int(spec.V)
        if self.min_length < 0:
            raise ValueError('min_length must be >= 0, got %d' % self.min_length)
        if self.no_repeat_ngram < 0:
            raise ValueError('no_repeat_ngram must be >= 0, got %d' % self.no_repeat_ngram)
        if self.ngram_stride < 1:
            raise ValueError('ngram_stride must be >= 1, got %d' % self.ngram_stride)
        if self.no_repeat_ngram % self.ngram_stride:
            raise ValueError('no_repeat_ngram %d is no multiple of ngram_stride %d' % (self.no_repeat_ngram, self.ngram_stride))
        if len(self.suppress) > self.MAX_SUPPRESS:
            raise ValueError('suppress holds %d ids, at most %d' % (len(self.suppress), self.MAX_SUPPRESS))
        for v in self.suppress:
            if not 0 <= v < V:
                raise ValueError('suppress: id %d is outside the vocabulary of %d' % (v, V))
            if v == spec.end_id:
                raise ValueError('suppress: end_id %d cannot be suppressed' % v)
        if self.min_length >= max_steps:
            raise ValueError('min_length %d is not below max_steps %d' % (self.min_length, max_steps))
        if (V + 31) // 32 > self.MAX_WORDS:
            raise ValueError('V = %d: constraints need a vocabulary of at most %d' % (V, 32 * self.MAX_WORDS))
        need = int(beam) + len(self.suppress) + 1 + int(max_steps)
        if V < need:
            raise ValueError('V = %d is too small: beam %d + %d suppress + 1 + max_steps %d = %d candidates are needed'
                             % (V, beam, len(self.suppress), max_steps, need))

    def c_struct(self):
        c = L.BeamConstraints()
        c.min_length, c.no_repeat_ngram, c.ngram_stride = self.min_length, self.no_repeat_ngram, self.ngram_stride
        c.n_suppress = len(self.suppress)
        for k, v in enumerate(self.suppress):
            c.suppress[k] = v
        return c


def constraints_from_config(c):
    """The BeamConstraints a configuration asks for, or None when it asks for none.  infer_min_length and
    infer_no_repeat_ngram count WORDS for `word` and `radix` tokens -- a radix word is len(number_to_base(len(wtoi),
    radix_base)) tokens, so both are multiplied by that length and the n-gram windows are aligned to it -- and characters
    for `char` tokens.  infer_suppress_words (a sequence or a comma-separated string) maps through wtoi; with radix tokens
    a word is not a token and the field is refused."""
    m, n, sup = (getattr(c, k, None) for k in ('infer_min_length', 'infer_no_repeat_ngram', 'infer_suppress_words'))
    if isinstance(sup, str):
        sup = [w for w in sup.split(',') if w]
    if not m and not n and not sup:
        return None
    m, n, stride = int(m or 0), int(n or 0), 1
    if c.token_type == 'radix':
        if sup:
            raise ValueError('infer_suppress_words: a word is not a token with radix tokens, words cannot be suppressed')
        stride = len(number_to_base(len(c.wtoi), c.radix_base))
        m, n = m * stride, n * stride
    ids = []
    for w in sup or ():
        if w not in c.wtoi:
            raise ValueError('infer_suppress_words: `%s` is not in the vocabulary' % (w,))
        ids.append(int(c.wtoi[w]))
    return BeamConstraints(min_length=m, no_repeat_ngram=n, ngram_stride=stride, suppress=ids)


def constraints_dir_suffix(c):
    """'_min{m}_ngram{n}_sup{k}' when the configuration sets any constraint field (in its own units), else ''."""
    m, n, sup = (getattr(c, k, None) for k in ('infer_min_length', 'infer_no_repeat_ngram', 'infer_suppress_words'))
    if m is None and n is None and sup is None:
        return ''
    if isinstance(sup, str):
        sup = [w for w in sup.split(',') if w]
    return '_min%d_ngram%d_sup%d' % (int(m or 0), int(n or 0), len(sup or ()))


class BeamGroups(_Keyed):
    """Diverse beam search (comic_beam_groups; Vijayakumar et al. 2016 with the Hamming diversity; extends
    rnn_decoder_beam_search, ops_rnn.py:49-112): the beam is split into `groups` groups of beam / groups slots, decided in
    order at every step; a later group ranks a candidate token by its score minus `diversity` times the number of slots of
    the earlier groups that chose that token at this step.  <EOS> and finished beams are never penalised; the beam state
    keeps the unpenalised log-probability.  Group 0 is plain beam search of width beam / groups.  The penalty is per TOKEN
    at the same position: with radix tokens it is not per word.  Immutable and hashable: decode contexts are keyed by it."""

    def __init__(self, groups=1, diversity=0.0):
        self.groups, self.diversity = int(groups), float(diversity)

    def key(self):
        return (self.groups, self.diversity)

    def __repr__(self):
        return 'BeamGroups(groups=%d, diversity=%r)' % self.key()

    @property
    def active(self):
        return self.groups > 1

    def check(self, beam, V=None):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field."""
        beam = int(beam)
        if self.groups < 1:
            raise ValueError('groups must be >= 1, got %d' % self.groups)
        if self.groups > beam:
            raise ValueError('groups %d exceeds the beam width %d' % (self.groups, beam))
        if beam % self.groups:
            raise ValueError('groups %d does not divide the beam width %d' % (self.groups, beam))
        if not (self.diversity >= 0.0) or math.isinf(self.diversity):
            raise ValueError('diversity must be finite and >= 0, got %r' % self.diversity)
        if V is not None and beam // self.groups > int(V):
            raise ValueError('groups: a group of %d slots exceeds the vocabulary of %d' % (beam // self.groups, V))

    def c_struct(self):
        g = L.BeamGroups()
        g.groups, g.diversity = self.groups, self.diversity
        return g

    def final_log_probs(self, scores, step_ids, lengths, end_id, lpw=0.0):
        """The beams' unpenalised total log-probabilities [B,W] after the last executed step, recovered on the host from
        that step's `scores` row (the ranks) and words: rank + diversity * count where the last word was penalised,
        times the length penalty's divisor.  Exact wherever no penalty applied (every finished caption without a length
        penalty); to fp32 rounding elsewhere."""
        sc, words = np.asarray(scores[-1], np.float32), np.asarray(step_ids[-1])
        B, W = words.shape
        Wg = W // self.groups
        count = np.zeros((B, W), np.float32)
        for w in range(Wg, W):
            before = words[:, :(w // Wg) * Wg]
            count[:, w] = (before == words[:, w:w + 1]).sum(axis=1)
        count[words == end_id] = 0
        out = sc + np.float32(self.diversity) * count
        if lpw:
            out = out * (((5.0 + np.asarray(lengths, np.float32)) / 6.0) ** np.float32(lpw))
        return out.astype(np.float32)


def groups_from_config(c):
    """The BeamGroups a configuration asks for (infer_beam_groups, infer_diversity), or None when it sets neither."""
    g, d = getattr(c, 'infer_beam_groups', None), getattr(c, 'infer_diversity', None)
    if g is None and d is None:
        return None
    grp = BeamGroups(groups=1 if g is None else g, diversity=0.0 if d is None else d)
    grp.check(c.infer_beam_size)
    return grp


def groups_dir_suffix(c):
    """'_grp{G}_div{diversity:g}' when the configuration sets a group field, else ''."""
    g, d = getattr(c, 'infer_beam_groups', None), getattr(c, 'infer_diversity', None)
    if g is None and d is None:
        return ''
    return '_grp%d_div%g' % (int(1 if g is None else g), float(0.0 if d is None else d))


class BeamRequired(_Keyed):
    """Beam search with required words (comic_beam_required; Anderson et al. 2017, the bank form of Post & Vilar 2018;
    extends rnn_decoder_beam_search, ops_rnn.py:49-112).  ids: int32 [B, C, S], -1 padded: row (b, q) is the S tokens of
    required word q of image b (S = 1 for word tokens, the radix word length for radix tokens), or all -1.  The beam is
    split into C*S + 1 banks by how much of the set a hypothesis has produced; slot c * (beam / banks) of a result is bank
    c's best, and the caption is the best of the highest bank that holds a finished-scoring hypothesis.  Hashable by
    (C, S) only: the table lives in device memory and is written in front of every launch or replay, so decode contexts
    and captured graphs are shared across tables."""
    MAX_WORDS, MAX_STRIDE = 4, 4

    def __init__(self, ids):
        self.ids = np.ascontiguousarray(np.asarray(ids, np.int32))
        if self.ids.ndim != 3:
            raise ValueError('required: ids must be [B, n_words, stride], got shape %r' % (self.ids.shape,))
        self.n_words, self.stride = int(self.ids.shape[1]), int(self.ids.shape[2])

    def key(self):
        return (self.n_words, self.stride)

    def __repr__(self):
        return 'BeamRequired(n_words=%d, stride=%d, images=%d)' % (self.n_words, self.stride, self.ids.shape[0])

    @property
    def active(self):
        return True

    @property
    def banks(self):
        return self.n_words * self.stride + 1

    def ctx_key(self):
        return ('required',) + self.key()

    def check(self, spec, beam, batch=None, max_steps=None, constraints=None, groups=None, sampling=None):
        """The rules of the C side and of the table, on the host before any GPU call; raises ValueError naming the field."""
        V, beam = int(spec.V), int(beam)
        if not 1 <= self.n_words <= self.MAX_WORDS:
            raise ValueError('required: n_words must be in [1,%d], got %d' % (self.MAX_WORDS, self.n_words))
        if not 1 <= self.stride <= self.MAX_STRIDE:
            raise ValueError('required: stride must be in [1,%d], got %d' % (self.MAX_STRIDE, self.stride))
        if beam % self.banks or not 1 <= beam <= 64:
            raise ValueError('required: %d banks (n_words %d * stride %d + 1) do not divide the beam width %d'
                             % (self.banks, self.n_words, self.stride, beam))
        if batch is not None and self.ids.shape[0] != int(batch):
            raise ValueError('required: the table holds %d images, the batch %d' % (self.ids.shape[0], int(batch)))
        if V > 65536:
            raise ValueError('required: V = %d exceeds 65536' % V)
        pad = self.ids[:, :, 0] < 0
        if ((self.ids < 0) != pad[:, :, None]).any():
            raise ValueError('required: a word is -1 in all of its tokens or in none')
        if (self.ids >= V).any():
            raise ValueError('required: token %d is outside the vocabulary of %d' % (int(self.ids.max()), V))
        if (self.ids == spec.end_id).any():
            raise ValueError('required: end_id %d cannot be required' % spec.end_id)
        if groups is not None and groups.groups > 1:
            raise ValueError('required words do not combine with beam groups (groups=%d)' % groups.groups)
        if sampling is not None and sampling.active:
            raise ValueError('required words do not combine with sampling')
        if constraints is not None and constraints.active and max_steps is not None:
            need = beam + len(constraints.suppress) + 1 + int(max_steps) + self.MAX_WORDS
            if V < need:
                raise ValueError('V = %d is too small: beam %d + %d suppress + 1 + max_steps %d + %d required = %d candidates '
                                 'are needed' % (V, beam, len(constraints.suppress), max_steps, self.MAX_WORDS, need))

    def c_struct(self):
        r = L.BeamRequired()
        r.n_words, r.stride = self.n_words, self.stride
        return r

    def result(self, last_scores):
        """(best_slot [B], met [B]) from the last executed step's scores [B, W]: the first slot of the highest bank whose
        first slot has a finite score, and the number of required words (padding included) that bank stands for."""
        sc = np.asarray(last_scores)
        Wb = sc.shape[1] // self.banks
        ok = np.isfinite(sc[:, ::Wb])                                            # [B, banks]
        bank = np.where(ok.any(axis=1), self.banks - 1 - np.argmax(ok[:, ::-1], axis=1), 0)
        return (bank * Wb).astype(np.int64), (bank // self.stride).astype(np.int64)


def required_image_key(filename):
    """The key of an image in --infer_require_file besides its file name: the image_id infer_fn derives from the name
    (the COCO number, or the base name without `.jpg` for names that hold an `@`), as a string; None when it has none."""
    import re
    image_id = filename.replace('.jpg', '')
    if '@' in image_id:
        return os.path.basename(image_id)
    found = re.findall(r'(?<=_)\d+', image_id)
    return str(int(found[0])) if found else None


def config_wtoi(c):
    """The word -> index map of a configuration: c.wtoi, or, before the input manager has read the vocabulary, the same
    file."""
    wtoi = getattr(c, 'wtoi', None)
    if wtoi is None:
        with open(os.path.join(c.dataset_dir, 'captions', c.dataset_file_pattern.format('wtoi')) + '.json') as f:
            wtoi = json.load(f)
    return wtoi


def word_stride(c, wtoi):
    """Tokens per word: 1 for `word` tokens, the radix word length for `radix` tokens."""
    return len(number_to_base(len(wtoi), c.radix_base)) if c.token_type == 'radix' else 1


def word_encoding(c, wtoi):
    """word -> list of word_stride tokens, for `word` and `radix` tokens (required words, the consensus idf table)."""
    if c.token_type == 'radix':
        from .ops import build_radix_wtoi
        return build_radix_wtoi(wtoi, c.radix_base)
    return {w: [int(i)] for w, i in wtoi.items()}


def required_from_config(c, filenames=None):
    """The required words a configuration asks for (infer_require_file, infer_require_words), or None when it names no
    file.  The file is JSON: image file name (with or without its directory) or image_id -> list of words.  Words map
    through wtoi for `word` tokens and through the radix encoding for `radix` tokens (`char` tokens are refused); words
    outside the vocabulary, <GO> / <EOS> / <PAD>, repeats and words beyond C = infer_require_words (default: the longest list
    in the file, at most 4) are dropped and reported.  infer_beam_size must be a multiple of C*S + 1.
    filenames None: the checks alone -> dict(n_words, stride, banks).  Else -> dict(n_words, stride, banks, required (a
    BeamRequired over all the images, in order), words, dropped (lists of words per image)); one summary line is printed."""
    path = getattr(c, 'infer_require_file', None)
    if not path:
        return None
    if c.token_type == 'char':
        raise ValueError('infer_require_file: required words need `word` or `radix` tokens, not `char`')
    with open(path) as f:
        table = json.load(f)
    if not isinstance(table, dict) or not all(isinstance(v, list) for v in table.values()):
        raise ValueError('infer_require_file: %s must hold a JSON object of image -> list of words' % path)
    C_ = getattr(c, 'infer_require_words', None)
    if C_ is None:
        C_ = max(1, min(BeamRequired.MAX_WORDS, max([len(v) for v in table.values()] or [1])))
    C_ = int(C_)
    if not 1 <= C_ <= BeamRequired.MAX_WORDS:
        raise ValueError('infer_require_words must be in [1,%d], got %d' % (BeamRequired.MAX_WORDS, C_))
    wtoi = config_wtoi(c)
    S = word_stride(c, wtoi)
    if S > BeamRequired.MAX_STRIDE:
        raise ValueError('infer_require_file: a radix word of %d tokens exceeds %d' % (S, BeamRequired.MAX_STRIDE))
    banks = C_ * S + 1
    if int(c.infer_beam_size) % banks:
        raise ValueError('infer_beam_size %d is no multiple of %d (infer_require_words %d * %d tokens per word + 1 banks)'
                         % (int(c.infer_beam_size), banks, C_, S))
    out = dict(n_words=C_, stride=S, banks=banks)
    if filenames is None:
        return out
    enc = word_encoding(c, wtoi)
    ids = np.full((len(filenames), C_, S), -1, np.int32)
    words, dropped = [], []
    for k, f in enumerate(filenames):
        asked = None
        for key in (f, os.path.basename(f), required_image_key(f)):
            if key is not None and key in table:
                asked = table[key]
                break
        keep, drop = [], []
        for w in asked or []:
            w = str(w)
            if w in ('<GO>', '<EOS>', '<PAD>') or w not in enc or w in keep or len(keep) == C_:
                drop.append(w)
            else:
                ids[k, len(keep)] = enc[w]
                keep.append(w)
        words.append(keep)
        dropped.append(drop)
    print('INFO: required words: %d of %d images name words; %d words kept, %d dropped (outside the vocabulary, repeated '
          'or beyond %d per image)' % (sum(1 for w in words if w), len(filenames), sum(len(w) for w in words),
                                       sum(len(d) for d in dropped), C_))
    out.update(required=BeamRequired(ids), words=words, dropped=dropped)
    return out


def required_dir_suffix(c):
    """'_req{C}_{stem of the file}' when the configuration names infer_require_file, else ''."""
    path = getattr(c, 'infer_require_file', None)
    if not path:
        return ''
    return '_req%d_%s' % (required_from_config(c)['n_words'], os.path.splitext(os.path.basename(path))[0])


class BeamPrefix(_Keyed):
    """Forced-prefix decoding (comic_beam_prefix; extends rnn_decoder_beam_search, ops_rnn.py:49-112).  ids: int32 [B, P],
    padded with -1 at the end of each row: the tokens (not words: a radix word is S tokens) the caption of image b must
    start with.  The length of a row is the index of its first -1; it may be 0 and differs per image.  Hashable by P only:
    the table lives in device memory and is written in front of every launch or replay, so one decode context and one
    captured graph serve every table of a width."""
    MAX_V = 65536

    def __init__(self, ids):
        self.ids = np.ascontiguousarray(np.asarray(ids, np.int32))
        self.max_tokens = int(self.ids.shape[1]) if self.ids.ndim == 2 else 0

    def key(self):
        return (self.max_tokens,)

    def __repr__(self):
        return 'BeamPrefix(max_tokens=%d, images=%d)' % (self.max_tokens, self.ids.shape[0] if self.ids.ndim else 0)

    @property
    def active(self):
        return True

    def ctx_key(self):
        return ('prefix',) + self.key()

    @property
    def lengths(self):
        """[B]: the index of the first -1 of each row (P for a full row)."""
        pad = self.ids < 0
        return np.where(pad.any(axis=1), pad.argmax(axis=1), self.ids.shape[1]).astype(np.int64)

    def check(self, spec, beam=None, batch=None, max_steps=None):
        """The rules of the C side and of the table, on the host before any GPU call; raises ValueError naming the field."""
        V = int(spec.V)
        if self.ids.ndim != 2:
            raise ValueError('prefix: ids must be [B, max_tokens], got shape %r' % (self.ids.shape,))
        if batch is not None and self.ids.shape[0] != int(batch):
            raise ValueError('prefix: the table holds %d images, the batch %d' % (self.ids.shape[0], int(batch)))
        if self.max_tokens < 1 or (max_steps is not None and self.max_tokens >= int(max_steps)):
            raise ValueError('prefix: max_tokens %d is outside [1,%s)'
                             % (self.max_tokens, 'max_steps' if max_steps is None else int(max_steps)))
        if V > self.MAX_V:
            raise ValueError('prefix: V = %d exceeds %d' % (V, self.MAX_V))
        pad = self.ids < 0
        if (pad[:, :-1] & ~pad[:, 1:]).any():
            raise ValueError('prefix: a -1 is followed by a token (rows are padded at the end only)')
        if (self.ids >= V).any():
            raise ValueError('prefix: token %d is outside the vocabulary of %d' % (int(self.ids.max()), V))
        if (self.ids == spec.end_id).any():
            raise ValueError('prefix: end_id %d cannot be part of a prefix' % spec.end_id)
        if (self.ids == spec.start_id).any():
            raise ValueError('prefix: start_id %d cannot be part of a prefix' % spec.start_id)

    def c_struct(self):
        r = L.BeamPrefix()
        r.max_tokens = self.max_tokens
        return r

    def prefix_log_probs(self, out, length_penalty_weight=0.0, groups=None, end_id=None):
        """[B, W] float32 from a beam_search result `out`: log p(prefix | image) of every slot's caption, the sum of its
        forced steps' log-probabilities -- the total its ancestor held after step len - 1, read from the result's
        `scores` through `parent_ids` with no launch.  0 for an image without a prefix.  `scores` are penalised ranks under
        a length penalty or beam groups: the divisor ((5 + len) / 6)^lpw and the diversity penalty lambda * count of the
        step are taken out again."""
        sc, par, ids = (np.asarray(out[k]) for k in ('scores', 'parent_ids', 'step_ids'))
        T, B, W = sc.shape
        lpw = float(length_penalty_weight or 0.0)
        n = np.minimum(self.lengths, T)                                # [B]
        if not n.any():
            return np.zeros((B, W), np.float32)
        rows = np.arange(B)[:, None]
        slot = np.tile(np.arange(W), (B, 1))                           # the ancestor of every final slot, step by step
        for t in range(T - 1, int(n.min()) - 1, -1):
            slot = np.where((t >= n)[:, None], par[t][rows, slot], slot)       # (executed steps: parents in [0, W))
        last = np.maximum(n - 1, 0)[:, None]                           # the last forced step of every image
        v = sc[last, rows, slot].astype(np.float32)
        if groups is not None and groups.groups > 1 and groups.diversity:
            Wg = W // groups.groups
            tok = ids[last, rows, np.arange(W)[None, :]]               # [B, W]: the words of that step, slot by slot
            mine = np.take_along_axis(tok, slot, axis=1)
            before = np.arange(W)[None, None, :] < ((slot // Wg) * Wg)[:, :, None]
            count = ((tok[:, None, :] == mine[:, :, None]) & before).sum(axis=2) * (mine != end_id)
            v = v + np.float32(groups.diversity) * count.astype(np.float32)
        if lpw:
            v = v * (((5.0 + n.astype(np.float32)) / 6.0) ** np.float32(lpw))[:, None]
        return np.where((n > 0)[:, None], v, np.float32(0.0)).astype(np.float32)


def prefix_words(c):
    """The --infer_prefix string of a configuration as its list of words ([] when it is not given)."""
    text = getattr(c, 'infer_prefix', None)
    return [] if not text else str(text).split()


def prefix_from_config(c, filenames=None, max_steps=None):
    """The forced prefixes a configuration asks for (infer_prefix: one string for every image; infer_prefix_file: JSON,
    image file name or image_id -> string or list of words, found by the keys of infer_require_file), or None when it names
    neither.  Both is a ValueError.  Words map through word_encoding (`word` and `radix` tokens; `char` tokens are refused).
    With infer_prefix a word outside the vocabulary or a special token is a ValueError that names it; in a file an image's
    prefix is cut before its first such word and the cut words are reported.
    filenames None: the checks alone -> dict(stride).  Else -> dict(stride, prefix (a BeamPrefix over all the images, in
    order; P is the longest prefix of the run), words, cut (lists of words per image)).  max_steps: P >= max_steps is a
    ValueError."""
    text, path = getattr(c, 'infer_prefix', None), getattr(c, 'infer_prefix_file', None)
    if not text and not path:
        return None
    if text and path:
        raise ValueError('infer_prefix and infer_prefix_file: give one of them, not both')
    flag = 'infer_prefix' if text else 'infer_prefix_file'
    if c.token_type == 'char':
        raise ValueError('%s: a forced prefix needs `word` or `radix` tokens, not `char`' % flag)
    wtoi = config_wtoi(c)
    S = word_stride(c, wtoi)
    enc = word_encoding(c, wtoi)
    special = ('<GO>', '<EOS>', '<PAD>')
    table = None
    if text:
        fixed = prefix_words(c)
        for w in fixed:
            if w in special or w not in enc:
                raise ValueError('infer_prefix: %r is %s' % (w, 'a special token' if w in special else 'outside the vocabulary'))
        longest = len(fixed)
    else:
        with open(path) as f:
            table = json.load(f)
        if not isinstance(table, dict) or not all(isinstance(v, (str, list)) for v in table.values()):
            raise ValueError('infer_prefix_file: %s must hold a JSON object of image -> string or list of words' % path)
        table = {k: (v.split() if isinstance(v, str) else [str(w) for w in v]) for k, v in table.items()}
        longest = max([len(v) for v in table.values()] or [0])
    out = dict(stride=S)
    if max_steps is not None and text and longest * S >= int(max_steps):
        raise ValueError('infer_prefix: %d tokens do not leave a step of the %d for the caption' % (longest * S, int(max_steps)))
    if filenames is None:
        return out
    words, cut = [], []
    for f in filenames:
        asked = fixed if text else None
        if table is not None:
            for key in (f, os.path.basename(f), required_image_key(f)):
                if key is not None and key in table:
                    asked = table[key]
                    break
        asked = list(asked or [])
        n = next((k for k, w in enumerate(asked) if w in special or w not in enc), len(asked))
        words.append(asked[:n])
        cut.append(asked[n:])
    P = max(1, max(len(w) for w in words) * S) if words else 1
    if max_steps is not None and P >= int(max_steps):
        raise ValueError('%s: the longest prefix, %d tokens, does not leave a step of the %d for the caption'
                         % (flag, P, int(max_steps)))
    ids = np.full((len(filenames), P), -1, np.int32)
    for k, w in enumerate(words):
        toks = [t for x in w for t in enc[x]]
        ids[k, :len(toks)] = toks
    print('INFO: forced prefix: %d of %d images start from a prefix, %d tokens at the most; %d words cut (outside the '
          'vocabulary or special)' % (sum(1 for w in words if w), len(filenames), P, sum(len(x) for x in cut)))
    out.update(prefix=BeamPrefix(ids), words=words, cut=cut)
    return out


def prefix_dir_suffix(c):
    """'_pfx_{words joined by -}' for infer_prefix, '_pfx_{stem of the file}' for infer_prefix_file, else ''."""
    text, path = getattr(c, 'infer_prefix', None), getattr(c, 'infer_prefix_file', None)
    if text and path:
        raise ValueError('infer_prefix and infer_prefix_file: give one of them, not both')
    if text:
        return '_pfx_' + '-'.join(prefix_words(c))
    if path:
        return '_pfx_' + os.path.splitext(os.path.basename(path))[0]
    return ''


class BeamSampling(_Keyed):
    """Sampling inside the beam step (comic_beam_sampling; extends rnn_decoder_beam_search, ops_rnn.py:49-112): the `beam`
    slots of an image are `beam` independent chains, each drawn from the step distribution at `temperature` by the
    Gumbel-max rule, with noise from a counter-based generator keyed by (seed, the image's index in the run, slot, step,
    token).  The beam state is the chain's log p(caption | image) under the model: unperturbed and untempered.  The
    temperature is part of a decode context's key (it is baked into the captured graph); the seed is not: it lives in a
    device tensor that is written in front of every launch or replay.  enabled=False is the inactive value."""

    def __init__(self, temperature=1.0, seed=0, enabled=True):
        self.temperature, self.seed, self.enabled = float(temperature), int(seed), bool(enabled)

    def key(self):
        return (self.temperature, self.seed, self.enabled)

    def __repr__(self):
        return 'BeamSampling(temperature=%r, seed=%d%s)' % (self.temperature, self.seed, '' if self.enabled else ', enabled=False')

    @property
    def active(self):
        return self.enabled

    def ctx_key(self):
        """What a decode context is keyed by: the temperature as the fp32 value the kernels see; not the seed."""
        return ('sample', float(np.float32(self.temperature)))

    def check(self, beam, length_penalty_weight=0.0, groups=None):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field."""
        with np.errstate(all='ignore'):
            t = np.float32(self.temperature)
            inv = np.float32(1.0) / t
        if not (np.isfinite(t) and t > 0):
            raise ValueError('temperature must be finite and > 0, got %r' % self.temperature)
        if not np.isfinite(inv):
            raise ValueError('temperature %r has no finite fp32 reciprocal' % self.temperature)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError('seed must be in [0, 2^64), got %d' % self.seed)
        if not self.enabled:
            return
        if not 1 <= int(beam) <= 64:
            raise ValueError('sampling: the number of samples (beam) must be in [1,64], got %d' % int(beam))
        if length_penalty_weight:
            raise ValueError('sampling does not combine with a length penalty (length_penalty_weight=%r)'
                             % length_penalty_weight)
        if groups is not None and groups.groups > 1:
            raise ValueError('sampling does not combine with beam groups (groups=%d)' % groups.groups)

    def c_struct(self, seed_dev):
        """seed_dev: the address of the device uint64[2] {seed, image_base}."""
        g = L.BeamSampling()
        g.temperature, g.seed_dev = self.temperature, seed_dev
        return g

    def seed_words(self, image_base=0):
        """{seed, image_base} as the int64 view of the device's uint64[2]."""
        if not 0 <= int(image_base) < 2 ** 64:
            raise ValueError('image_base must be in [0, 2^64), got %d' % int(image_base))
        return np.array([self.seed, int(image_base)], np.uint64).view(np.int64)


def sampling_from_config(c):
    """The BeamSampling a configuration asks for (infer_sample, infer_temperature, infer_sample_seed), or None when it
    sets none of them; inactive unless infer_sample is set."""
    on, t, seed = (getattr(c, k, None) for k in ('infer_sample', 'infer_temperature', 'infer_sample_seed'))
    if not on and t is None and seed is None:
        return None
    smp = BeamSampling(temperature=1.0 if t is None else t, seed=0 if seed is None else seed, enabled=bool(on))
    smp.check(c.infer_beam_size, getattr(c, 'infer_length_penalty_weight', 0.0) or 0.0, groups_from_config(c))
    return smp


def sampling_dir_suffix(c):
    """'_smp_t{temperature:g}_s{seed}' when the configuration sets infer_sample, else ''."""
    if not getattr(c, 'infer_sample', None):
        return ''
    t, seed = getattr(c, 'infer_temperature', None), getattr(c, 'infer_sample_seed', None)
    return '_smp_t%g_s%d' % (float(1.0 if t is None else t), int(0 if seed is None else seed))


class BeamTruncation(_Keyed):
    """Top-k and nucleus (top-p) truncation of the sampled step (comic_beam_truncation; extends rnn_decoder_beam_search,
    ops_rnn.py:49-112): a live slot draws from the `top_k` likeliest tokens of the tempered step distribution only
    (0 = off; ties by lowest id), and of those from the smallest set of likeliest tokens whose probability, renormalised
    over them, reaches `top_p` (>= 1 = off; tokens tied at the boundary all stay) -- the temperature -> top-k -> top-p
    order.  Constraints are applied first: a banned token counts neither in k nor in the mass.  The log-probabilities a
    decode returns stay the model's own unperturbed, untempered, UNTRUNCATED log p(caption | image), which Decoder.score
    reproduces; they are not the log-probability under the truncated distribution.  Both values are baked into a
    captured graph, so both are part of a decode context's key.  BeamTruncation() is the inactive value."""

    def __init__(self, top_k=0, top_p=1.0):
        self.top_k, self.top_p = int(top_k), float(top_p)

    def key(self):
        return (self.top_k, self.top_p)

    def __repr__(self):
        return 'BeamTruncation(top_k=%d, top_p=%r)' % self.key()

    @property
    def active(self):
        return self.top_k >= 1 or self.top_p < 1.0

    def ctx_key(self):
        """What a decode context is keyed by: top_k, and top_p as the fp32 value the kernel sees."""
        return ('truncate', self.top_k, float(np.float32(self.top_p)))

    def check(self, sampling=None):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field.  An active
        truncation needs an active BeamSampling."""
        if self.top_k < 0:
            raise ValueError('top_k must be >= 0, got %d' % self.top_k)
        if not self.top_p > 0.0:
            raise ValueError('top_p must be > 0 and not NaN, got %r' % self.top_p)
        if self.active and (sampling is None or not sampling.active):
            raise ValueError('truncation (top_k / top_p) applies to sampling only: it needs an active BeamSampling')

    def c_struct(self):
        g = L.BeamTruncation()
        g.top_k, g.top_p = self.top_k, self.top_p
        return g


def truncation_from_config(c):
    """The BeamTruncation a configuration asks for (infer_top_k, infer_top_p), or None when it sets neither; either of
    them without infer_sample is a ValueError."""
    k, p = getattr(c, 'infer_top_k', None), getattr(c, 'infer_top_p', None)
    if k is None and p is None:
        return None
    if not getattr(c, 'infer_sample', None):
        raise ValueError('infer_top_k / infer_top_p apply to sampling only: set infer_sample')
    trc = BeamTruncation(top_k=0 if k is None else k, top_p=1.0 if p is None else p)
    trc.check(sampling_from_config(c))
    return trc


def truncation_dir_suffix(c):
    """'_k{top_k}_p{top_p:g}' when the configuration samples under a truncation -- a stage that is off is left out:
    '_k40', '_p0.9' -- else ''."""
    if not getattr(c, 'infer_sample', None):
        return ''
    k, p = getattr(c, 'infer_top_k', None), getattr(c, 'infer_top_p', None)
    out = ''
    if k is not None and int(k) >= 1:
        out += '_k%d' % int(k)
    if p is not None and float(p) < 1.0:
        out += '_p%g' % float(p)
    return out


def _splitmix64(z):
    """csrc/splitmix.h on a numpy uint64 array (wraps modulo 2^64)."""
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def ngram_keys(tokens):
    """The 64-bit keys of n n-grams of m tokens each (int array [n, m]; comic_caption_consensus): h = splitmix64(m), then
    h = splitmix64(h ^ token) token by token; a result of 0 becomes 1.  -> uint64 [n]."""
    tokens = np.asarray(tokens, np.int64)
    h = _splitmix64(np.full(tokens.shape[0], tokens.shape[1], np.uint64))
    for s in range(tokens.shape[1]):
        h = _splitmix64(h ^ tokens[:, s].astype(np.uint64))
    return np.where(h == 0, np.uint64(1), h)


class NgramIdf:
    """The idf table of the consensus selector in the form the device reads (comic_caption_consensus): uint64 keys[cap]
    (0 = empty) beside double g[cap], g = log(ref_len) - log(max(1, df)) formed here in double; open addressing with
    linear probing from key & (cap - 1), cap a power of two of at least twice the number of entries.  An n-gram the table
    does not hold gets log_ref_len.  kept / skipped count the n-grams of the source that went in / were left out."""

    def __init__(self, keys, g, log_ref_len, stride, kept=None, skipped=0):
        self.keys = np.ascontiguousarray(keys, np.uint64)
        self.g = np.ascontiguousarray(g, np.float64)
        self.cap = int(self.keys.shape[0])
        if self.cap < 1 or self.cap & (self.cap - 1) or self.g.shape != self.keys.shape:
            raise ValueError('idf: keys and g must share a power-of-two capacity, got %r and %r' % (self.keys.shape, self.g.shape))
        self.log_ref_len, self.stride = float(log_ref_len), int(stride)
        self.kept = int((self.keys != 0).sum()) if kept is None else int(kept)
        self.skipped = int(skipped)
        self._dev = {}

    def __repr__(self):
        return 'NgramIdf(%d n-grams in %d slots, stride=%d, %d skipped)' % (self.kept, self.cap, self.stride, self.skipped)

    @classmethod
    def from_document_frequency(cls, df, ref_len, encode, stride, special=('<GO>', '<EOS>', '<PAD>')):
        """df: {tuple of words: document count}; encode: word -> list of `stride` tokens (word_encoding).  N-grams that
        hold a word outside `encode` or one of `special` (<GO> / <EOS> / <PAD>) are skipped and counted."""
        stride = int(stride)
        log_ref_len = math.log(float(ref_len))
        by_len, skipped = {}, 0
        for ng, cnt in df.items():
            if any(w in special or w not in encode for w in ng):
                skipped += 1
                continue
            toks = [t for w in ng for t in encode[w]]
            if len(toks) != len(ng) * stride:
                raise ValueError('idf: the n-gram %r maps to %d tokens, not %d words of stride %d'
                                 % (ng, len(toks), len(ng), stride))
            rows, gs = by_len.setdefault(len(toks), ([], []))
            rows.append(toks)
            gs.append(log_ref_len - math.log(max(1.0, float(cnt))))
        key_list, g_list = [], []
        for m in sorted(by_len):
            rows, gs = by_len[m]
            key_list += ngram_keys(np.asarray(rows, np.int64).reshape(len(rows), m)).tolist()
            g_list += gs
        cap = 2
        while cap < 2 * len(key_list):
            cap *= 2
        keys, g, kept = [0] * cap, [0.0] * cap, 0
        for key, val in zip(key_list, g_list):
            at = key & (cap - 1)
            while keys[at] != 0 and keys[at] != key:
                at = (at + 1) & (cap - 1)
            if keys[at] == key:            # two n-grams, one 64-bit key: the first stays
                skipped += 1
                continue
            keys[at], g[at] = key, val
            kept += 1
        return cls(np.array(keys, np.uint64), np.array(g, np.float64), log_ref_len, stride, kept, skipped)

    @classmethod
    def from_pickle(cls, path, config):
        """The `{pattern}scst-words.p` file of scst/prepro_ngrams.py, through the configuration's vocabulary."""
        from .scst.scorers import load_df_pickle
        if config.token_type == 'char':
            raise ValueError('infer_consensus_df: the idf table needs `word` or `radix` tokens, not `char`')
        d = load_df_pickle(path)
        wtoi = config_wtoi(config)
        idf = cls.from_document_frequency(d['document_frequency'], d['ref_len'], word_encoding(config, wtoi),
                                          word_stride(config, wtoi))
        print('INFO: consensus idf: %d n-grams of %s kept, %d skipped (outside the vocabulary or with <GO> / <EOS> / <PAD>)'
              % (idf.kept, path, idf.skipped))
        return idf

    def device(self, torch, device):
        """(keys, g) as device tensors (the keys as the int64 view of the uint64 words); uploaded once per device."""
        t = self._dev.get(str(device))
        if t is None:
            t = self._dev[str(device)] = (torch.from_numpy(self.keys.view(np.int64)).to(device),
                                          torch.from_numpy(self.g).to(device))
        return t


class Consensus(_Keyed):
    """Consensus (minimum-Bayes-risk) selection among the W candidates of an image (comic_caption_consensus; no counterpart
    in common/ops_rnn.py): the utility of a candidate is its mean CIDEr-D similarity (n-grams of 1..4 words, sigma) to its
    siblings, weighted by `weights`: 'uniform' (the Monte-Carlo estimate, for samples) or 'posterior' (the softmax of the
    final log-probabilities over the slots, for n-best lists; a slot of -inf neither votes nor can be chosen).  stride: the
    tokens of a word (1 for `word` tokens, the radix word length for `radix`); idf: an NgramIdf or None (every n-gram
    weighs 1).  Immutable; hashable by (weights, stride, sigma, the table's identity)."""
    MODES = {'uniform': 0, 'posterior': 1}          # COMIC_CONSENSUS_*
    MAX_W, MAX_UNITS, MAX_STRIDE = 32, 64, 8

    def __init__(self, weights='uniform', stride=1, idf=None, sigma=6.0):
        self.weights, self.stride, self.idf, self.sigma = str(weights), int(stride), idf, float(sigma)

    def key(self):
        return (self.weights, self.stride, self.sigma, id(self.idf) if self.idf is not None else None)

    def __repr__(self):
        return 'Consensus(weights=%r, stride=%d, idf=%r, sigma=%r)' % (self.weights, self.stride, self.idf, self.sigma)

    def check(self, beam, max_steps):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field."""
        if self.weights not in self.MODES:
            raise ValueError("consensus: weights must be 'uniform' or 'posterior', got %r" % self.weights)
        if not 1 <= self.stride <= self.MAX_STRIDE:
            raise ValueError('consensus: stride must be in [1,%d], got %d' % (self.MAX_STRIDE, self.stride))
        if not (self.sigma > 0.0 and math.isfinite(self.sigma)):
            raise ValueError('consensus: sigma must be finite and > 0, got %r' % self.sigma)
        if self.idf is not None and self.idf.stride != self.stride:
            raise ValueError('consensus: the idf table was built for stride %d, not %d' % (self.idf.stride, self.stride))
        if not 1 <= int(beam) <= self.MAX_W:
            raise ValueError('consensus: the number of candidates (beam) must be in [1,%d], got %d' % (self.MAX_W, int(beam)))
        if not 1 <= int(max_steps) <= self.MAX_UNITS * self.stride:
            raise ValueError('consensus: max_steps = %d exceeds %d words of %d tokens'
                             % (int(max_steps), self.MAX_UNITS, self.stride))


def caption_consensus(lib, torch, ids, end_id, cons, log_probs=None, posterior=None):
    """One comic_caption_consensus launch on the device tensor ids [T, B, W] (int32, contiguous) -> device tensors
    (utility [B, W] float64, best [B] int32).  posterior: None follows cons.weights; True forces the posterior weights
    (log_probs [B, W] float32 on the device is then needed)."""
    T, B, W = (int(x) for x in ids.shape)
    cons.check(W, T)
    if posterior is None:
        posterior = cons.weights == 'posterior'
    if posterior and log_probs is None:
        raise ValueError("consensus: weights='posterior' needs log_probs")
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    if posterior:
        assert log_probs.dtype == torch.float32 and log_probs.is_contiguous() and tuple(log_probs.shape) == (B, W)
    util = torch.empty((B, W), dtype=torch.float64, device=ids.device)
    best = torch.empty(B, dtype=torch.int32, device=ids.device)
    if lib.comic_caption_consensus_workspace(B, W, T, cons.stride) != 0:
        raise L.ComicHipError('caption_consensus: the workspace query failed')
    keys, g = cons.idf.device(torch, ids.device) if cons.idf is not None else (None, None)
    L.check(lib.comic_caption_consensus(
        ids.data_ptr(), T, B, W, int(end_id), cons.stride, log_probs.data_ptr() if posterior else None, 1 if posterior else 0,
        L.ptr(keys), L.ptr(g), cons.idf.cap if cons.idf is not None else 0,
        cons.idf.log_ref_len if cons.idf is not None else 0.0, cons.sigma, util.data_ptr(), best.data_ptr(), None, 0,
        L.stream_ptr()), 'caption_consensus')
    return util, best


def _attach_consensus(dec, out, pred, cons, forced_posterior, last_scores, on_device):
    """The consensus launch of a beam_search on its device `pred` [T, B, W]; the result gains `consensus` [B, W] and
    `consensus_best` [B].  The posterior weights read the final log-probabilities: last_scores, the last executed row of
    the decode's device `scores`, where that is what the result reports (on_device); the host forms the others (beam
    groups, required words under a length penalty), and those [B, W] floats are uploaded."""
    torch = dec.torch
    posterior = forced_posterior or cons.weights == 'posterior'
    lp = None
    if posterior:
        lp = last_scores if on_device else \
            torch.from_numpy(np.ascontiguousarray(out['log_probs'], np.float32)).to(pred.device)
    util, best = caption_consensus(dec.lib, torch, pred, dec.spec.end_id, cons, lp, posterior)
    out['consensus'], out['consensus_best'] = util.cpu().numpy(), best.cpu().numpy()


def _baseline_ids(torch, base, device):
    """The reward's baseline rollout [T0,B] (a tensor, an array or None) as a contiguous int32 tensor on `device`."""
    if base is None:
        return None
    base = base if torch.is_tensor(base) else torch.from_numpy(np.ascontiguousarray(base, np.int32))
    return base.to(device=device, dtype=torch.int32).contiguous()


def _attach_reward(dec, out, pred, opts):
    """The reward launch of a beam_search on its device `pred` [T, B, W], right after the tree gather and outside the
    captured graph, as the consensus launch; the result gains `reward` [B, W'] float64 and `advantage` [W, B] float32
    (numpy) and keeps the device tensors of all five outputs in `reward_device` for the caller."""
    res = scst_reward(dec.lib, dec.torch, pred, opts.reward_refs, opts.reward,
                      _baseline_ids(dec.torch, opts.reward_baseline_ids, pred.device))
    out['reward_device'] = res
    out['reward'], out['advantage'] = res['reward'].cpu().numpy(), res['advantage'].cpu().numpy()


def _beam_outputs(ctx, torch, device, B, W, max_steps):
    """The beam executors' output buffers of a decode context (Decoder._infer_ctx, EnsembleDecoder._ctx)."""
    i32 = dict(dtype=torch.int32, device=device)
    # rows past the executed steps are never written (device-side early exit): poison them so a
    # kernel that indexes through them fails the same way every time
    ctx.step_ids = torch.full((max_steps, B, W), 0x7f7f7f7f, **i32)
    ctx.parent_ids = torch.full((max_steps, B, W), 0x7f7f7f7f, **i32)
    ctx.scores = torch.empty((max_steps, B, W), dtype=torch.float32, device=device)
    ctx.lengths = torch.empty((B, W), dtype=torch.int64, device=device)
    ctx.finished = torch.empty((B, W), **i32)
    ctx.steps = torch.empty(1, **i32)


def _unpenalised_totals(last_scores, lengths, lpw):
    """The final log-probabilities [B,W] from the last penalised scores: times the length penalty's divisor."""
    lp = last_scores.copy()
    if lpw:
        lp = (lp * (((5.0 + lengths.astype(np.float32)) / 6.0) ** np.float32(lpw))).astype(np.float32)
    return lp


def _beam_result(dec, ctx, B, W, opts, want_attention):
    """The result dict of a beam_search from its finished context: the tree gather, the fetches, what the options add
    (`groups`, `log_probs`, `banks`, `best_slot`, `met`), the consensus launch and the beam-sorted alignments (ctx.hist)."""
    torch, s, lpw = dec.torch, dec.spec, opts.length_penalty_weight
    grp, smp, rqd = opts.grp, opts.smp, opts.required
    T = int(ctx.steps.item())
    max_len = ctx.lengths.max(dim=1).values.to(torch.int32).contiguous()
    pred = torch.empty((T, B, W), dtype=torch.int32, device=dec.device)
    L.check(dec.lib.comic_gather_tree(ctx.step_ids[:T].data_ptr(), ctx.parent_ids[:T].data_ptr(), max_len.data_ptr(),
                                      pred.data_ptr(), T, B, W, s.end_id, L.stream_ptr()), 'gather_tree')
    par = ctx.parent_ids[:T].cpu().numpy()
    ln = ctx.lengths.cpu().numpy()
    out = dict(predicted_ids=pred.cpu().numpy(), scores=ctx.scores[:T].cpu().numpy(),
               step_ids=ctx.step_ids[:T].cpu().numpy(), parent_ids=par, lengths=ln, groups=1)
    if grp is not None:
        out['groups'] = grp.groups
        out['log_probs'] = grp.final_log_probs(out['scores'], out['step_ids'], ln, s.end_id, lpw)
    if smp is not None:                 # the state after the last executed step: a finished chain's carries over
        out['log_probs'] = out['scores'][-1].copy()
    if rqd is not None:
        out['log_probs'], out['banks'] = _unpenalised_totals(out['scores'][-1], ln, lpw), rqd.banks
        out['best_slot'], out['met'] = rqd.result(out['scores'][-1])
    if opts.prefix is not None:
        if 'log_probs' not in out:      # the plain beam
            out['log_probs'] = _unpenalised_totals(out['scores'][-1], ln, lpw)
        out['prefix_log_prob'] = opts.prefix.prefix_log_probs(out, lpw, grp, s.end_id)
    if opts.consensus is not None:
        _attach_consensus(dec, out, pred, opts.consensus, rqd is not None, ctx.scores[T - 1],
                          grp is None and not (rqd is not None and lpw))
    if opts.reward is not None:
        _attach_reward(dec, out, pred, opts)
    if want_attention:
        out['attn_hist'] = gather_tree_from_array(ctx.hist[:T].cpu().numpy(), par, ln, s.end_id)
    return out


def consensus_from_config(c, load_idf=True):
    """The Consensus a configuration asks for (infer_consensus, infer_consensus_df), or None when it sets neither: the
    uniform weights over the samples, the words of the configuration's token type, and the idf table of the
    `{pattern}scst-words.p` file infer_consensus_df names (without it every n-gram weighs 1).  `char` tokens,
    infer_consensus without infer_sample and infer_consensus_df without infer_consensus are ValueErrors.
    load_idf=False: the checks alone, the file is not read (the Consensus then carries no table)."""
    on, path = getattr(c, 'infer_consensus', None), getattr(c, 'infer_consensus_df', None)
    if not on and not path:
        return None
    if not on:
        raise ValueError('infer_consensus_df applies to the consensus selection only: set infer_consensus')
    if not getattr(c, 'infer_sample', None):
        raise ValueError('infer_consensus selects among samples: set infer_sample')
    if c.token_type == 'char':
        raise ValueError('infer_consensus: the consensus needs `word` or `radix` tokens, not `char`')
    S = word_stride(c, config_wtoi(c))
    if path and not os.path.isfile(path):
        raise ValueError('infer_consensus_df: %s is no file' % path)
    cons = Consensus('uniform', S, NgramIdf.from_pickle(path, c) if path and load_idf else None)
    cons.check(c.infer_beam_size, int(c.infer_max_length) * S)
    return cons


def consensus_dir_suffix(c):
    """'_cns' when the configuration sets infer_consensus, '_cns_df' when it names infer_consensus_df as well, else ''."""
    if not getattr(c, 'infer_consensus', None):
        return ''
    return '_cns_df' if getattr(c, 'infer_consensus_df', None) else '_cns'


class RewardVocab:
    """word -> word id for the device reward (comic_scst_reward): the ids of the configuration's wtoi, and, for a word
    outside it, an extended id >= len(wtoi), assigned on first sight and kept, one per distinct string.  Such a word matches
    among references and in the idf table and never a rollout: the kernel drops every rollout word id >= n_ids.
    n_ids: the ids that ops.id_to_caption(skip_unmapped=True) turns into text -- len(wtoi), less one where no word carries
    the id len(wtoi) - 1 ('-1' is <PAD>).  token_type / radix_base / word_len say how a rollout spells a word."""

    def __init__(self, config):
        if config.token_type == 'char':
            raise ValueError('scst_reward: the device reward needs `word` or `radix` tokens, not `char`')
        wtoi = config_wtoi(config)
        self.token_type = config.token_type
        self.radix_base = int(config.radix_base) if self.token_type == 'radix' else 0
        self.word_len = word_stride(config, wtoi)
        self.size = len(wtoi)
        self.ids = {w: int(i) for w, i in wtoi.items() if int(i) >= 0}
        # radix_ids_to_captions_and_ids's `simple` rule: joining and splitting the words of a caption must be the identity
        bad = [w for w in self.ids if not w or w.split() != [w]]
        if bad:
            raise ValueError('scst_reward: the vocabulary holds an empty word or one with white space (%r): text and word ids '
                             'would part' % bad[0])
        self.n_ids = self.size - (0 if (self.size - 1) in set(self.ids.values()) else 1)
        self.end_id = int(wtoi['<EOS>']) if self.token_type == 'word' else self.radix_base + 1
        self.extended = {}
        self._extended_from = max([self.size] + [i + 1 for i in self.ids.values()])      # beyond every id of the table

    def id(self, word):
        i = self.ids.get(word)
        if i is None:
            i = self.extended.get(word)
            if i is None:
                i = self.extended[word] = self._extended_from + len(self.extended)
        return i

    def encode(self, caption):
        """A caption's text -> the list of its word ids (str.split, as the host scorer's precook)."""
        return [self.id(w) for w in caption.split()]


class RewardRefs:
    """The reference captions of a batch in the form the device reward reads: refs int32 [B, R, Lr] of word ids, -1 padded,
    and n_refs int32 [B].  pack() builds it from the [[str]] an InputManager_SCST yields; device() uploads it once."""
    MAX_R, MAX_WORDS = 8, 64

    def __init__(self, refs, n_refs):
        self.refs = np.ascontiguousarray(refs, np.int32)
        self.n_refs = np.ascontiguousarray(n_refs, np.int32)
        if self.refs.ndim != 3 or self.n_refs.shape != self.refs.shape[:1]:
            raise ValueError('reward_refs: refs must be [B, R, Lr] and n_refs [B], got %r and %r'
                             % (self.refs.shape, self.n_refs.shape))
        self._dev = None

    @classmethod
    def pack(cls, refs, vocab):
        rows = [[vocab.encode(r) for r in rl] for rl in refs]
        if not rows or any(not rl for rl in rows):
            raise ValueError('reward_refs: every image needs at least one reference')
        R = max(len(rl) for rl in rows)
        Lr = max(1, max(len(r) for rl in rows for r in rl))
        if R > cls.MAX_R:
            raise ValueError('reward_refs: %d references of an image exceed %d' % (R, cls.MAX_R))
        if Lr > cls.MAX_WORDS:
            raise ValueError('reward_refs: a reference of %d words exceeds %d' % (Lr, cls.MAX_WORDS))
        out = np.full((len(rows), R, Lr), -1, np.int32)
        for b, rl in enumerate(rows):
            for r, ws in enumerate(rl):
                out[b, r, :len(ws)] = ws
        return cls(out, [len(rl) for rl in rows])

    def device(self, torch, device):
        if self._dev is None or self._dev[0] != str(device):
            self._dev = (str(device), torch.from_numpy(self.refs).to(device), torch.from_numpy(self.n_refs).to(device))
        return self._dev[1:]


class Reward(_Keyed):
    """The SCST reward on the device (comic_scst_reward; captionScorer.get_hypo_scores, common/scst/scorers.py:43-171):
    CIDEr-D * weights_ciderD + sum_k BLEU-k * weights_bleu[k] of every rollout against its image's references, and the
    advantage against `baseline`: 'none', 'greedy' (the reward of a baseline rollout) or 'mean' (the mean reward of the
    image's other rollouts: leave-one-out).  idf: an NgramIdf of stride 1 built through `vocab` (from_pickle) or None (every
    n-gram weighs 1); vocab: the RewardVocab the references are packed with.  Immutable; hashable by (weights, baseline,
    sigma, the identities of table and vocabulary)."""
    BASELINES = {'none': 0, 'greedy': 1, 'mean': 2}   # COMIC_SCST_BASELINE_*
    MAX_W, MAX_WORDS, MAX_WORD_LEN = 32, 64, 8

    def __init__(self, weights_ciderD=1.0, weights_bleu=(0.0, 0.0, 0.0, 0.0), idf=None, baseline='greedy', vocab=None,
                 sigma=6.0):
        self.weights_ciderD, self.weights_bleu = float(weights_ciderD), tuple(float(w) for w in weights_bleu)
        self.idf, self.baseline, self.vocab, self.sigma = idf, str(baseline), vocab, float(sigma)

    def key(self):
        return (self.weights_ciderD, self.weights_bleu, self.baseline, self.sigma, id(self.idf), id(self.vocab))

    def __repr__(self):
        return 'Reward(weights_ciderD=%r, weights_bleu=%r, idf=%r, baseline=%r)' % (
            self.weights_ciderD, self.weights_bleu, self.idf, self.baseline)

    @classmethod
    def from_pickle(cls, path, config, baseline='greedy', weights_ciderD=None, weights_bleu=None):
        """The Reward of a configuration: its vocabulary, its scst_weight_* (unless given) and the `{pattern}scst-words.p`
        file of scst/prepro_ngrams.py as a stride-1 word-id table.  Every n-gram of the file goes in: a word outside the
        vocabulary through its extended id, so that no reference n-gram loses its document frequency."""
        from .scst.scorers import load_df_pickle
        vocab = RewardVocab(config)
        d = path if isinstance(path, dict) else load_df_pickle(path)
        df = {(tuple(ng.split()) if isinstance(ng, str) else tuple(ng)): cnt for ng, cnt in d['document_frequency'].items()}
        encode = {w: [vocab.id(w)] for ng in df for w in ng}
        idf = NgramIdf.from_document_frequency(df, d['ref_len'], encode, 1, special=())
        wc = getattr(config, 'scst_weight_ciderD', 1.0) if weights_ciderD is None else weights_ciderD
        wb = getattr(config, 'scst_weight_bleu', (0.0,) * 4) if weights_bleu is None else weights_bleu
        return cls(wc, wb, idf, baseline, vocab)

    def check(self, beam, max_steps, baseline_steps=None):
        """The rules of the C side, on the host before any GPU call; raises ValueError naming the field."""
        if self.vocab is None:
            raise ValueError('reward: vocab is missing (a RewardVocab; Reward.from_pickle builds it)')
        if self.baseline not in self.BASELINES:
            raise ValueError("reward: baseline must be 'none', 'greedy' or 'mean', got %r" % self.baseline)
        if len(self.weights_bleu) != 4:
            raise ValueError('reward: weights_bleu must hold 4 weights, got %d' % len(self.weights_bleu))
        if not all(math.isfinite(w) for w in (self.weights_ciderD,) + self.weights_bleu):
            raise ValueError('reward: weights_ciderD and weights_bleu must be finite')
        if not (self.sigma > 0.0 and math.isfinite(self.sigma)):
            raise ValueError('reward: sigma must be finite and > 0, got %r' % self.sigma)
        if self.idf is not None and self.idf.stride != 1:
            raise ValueError('reward: the idf table must be built on word ids (stride 1), not stride %d' % self.idf.stride)
        wl = self.vocab.word_len
        if not 1 <= wl <= self.MAX_WORD_LEN:
            raise ValueError('reward: a word of %d tokens exceeds %d' % (wl, self.MAX_WORD_LEN))
        if not 1 <= int(beam) <= self.MAX_W:
            raise ValueError('reward: the number of rollouts (beam) must be in [1,%d], got %d' % (self.MAX_W, int(beam)))
        if self.baseline == 'mean' and int(beam) < 2:
            raise ValueError("reward: baseline 'mean' (leave-one-out) needs beam >= 2, got %d" % int(beam))
        if not 1 <= int(max_steps) <= self.MAX_WORDS * wl:
            raise ValueError('reward: max_steps = %d exceeds %d words of %d tokens' % (int(max_steps), self.MAX_WORDS, wl))
        if self.baseline == 'greedy' and baseline_steps is None:
            raise ValueError("reward: baseline 'greedy' needs baseline_ids")
        if baseline_steps is not None and not 1 <= int(baseline_steps) <= self.MAX_WORDS * wl:
            raise ValueError('reward: baseline_ids of %d steps exceed %d words of %d tokens'
                             % (int(baseline_steps), self.MAX_WORDS, wl))


def scst_reward(lib, torch, ids, refs, reward, baseline_ids=None, baseline_first_eos=None):
    """One comic_scst_reward launch on the device tensors ids [T, B, W] and baseline_ids [T0, B] or None (int32,
    contiguous; baseline_first_eos [B] int32: the greedy decode's first <EOS> positions, which bound the rows it wrote) against the RewardRefs `refs` -> dict of device tensors: cider [B, W'], bleu [B, W', 4], reward [B, W'],
    baseline [B, W] (float64) and advantage [W, B] (float32, hypothesis-major: the row order of the update)."""
    T, B, W = (int(x) for x in ids.shape)
    T0 = None if baseline_ids is None else int(baseline_ids.shape[0])
    reward.check(W, T, T0)
    v = reward.vocab
    assert ids.dtype == torch.int32 and ids.is_contiguous()
    if baseline_ids is not None:
        assert baseline_ids.dtype == torch.int32 and baseline_ids.is_contiguous() and tuple(baseline_ids.shape) == (T0, B)
    if refs.refs.shape[0] != B:
        raise ValueError('reward_refs: references of %d images for a batch of %d' % (refs.refs.shape[0], B))
    R, Lr = (int(x) for x in refs.refs.shape[1:])
    if lib.comic_scst_reward_workspace(B, W, int(T0 is not None), T, T0 or 0, v.word_len, R, Lr) < 0:
        raise ValueError('reward: %s' % lib.comic_last_error().decode())
    refs_dev, n_dev = refs.device(torch, ids.device)
    Wt = W + (T0 is not None)
    f64 = dict(dtype=torch.float64, device=ids.device)
    out = dict(cider=torch.empty((B, Wt), **f64), bleu=torch.empty((B, Wt, 4), **f64), reward=torch.empty((B, Wt), **f64),
               baseline=torch.empty((B, W), **f64), advantage=torch.empty((W, B), dtype=torch.float32, device=ids.device))
    keys, g = reward.idf.device(torch, ids.device) if reward.idf is not None else (None, None)
    L.check(lib.comic_scst_reward(
        ids.data_ptr(), T, B, W, L.ptr(baseline_ids), T0 or 0, L.ptr(baseline_first_eos), 1 if v.token_type == 'radix' else 0, v.end_id,
        v.radix_base, v.word_len, v.n_ids, refs_dev.data_ptr(), n_dev.data_ptr(), R, Lr, L.ptr(keys), L.ptr(g),
        reward.idf.cap if reward.idf is not None else 0, reward.idf.log_ref_len if reward.idf is not None else 0.0,
        reward.sigma, reward.weights_ciderD, (C.c_double * 4)(*reward.weights_bleu), Reward.BASELINES[reward.baseline],
        out['cider'].data_ptr(), out['bleu'].data_ptr(), out['reward'].data_ptr(), out['baseline'].data_ptr(),
        out['advantage'].data_ptr(), L.stream_ptr()), 'scst_reward')
    return out


def _active(option):
    return option if option is not None and option.active else None


@dataclass(frozen=True)
class BeamOptions:
    """Which decode a beam search is, as one immutable value (comic_beam_options; extends rnn_decoder_beam_search,
    ops_rnn.py:49-112): the length penalty, the five executor options, the consensus selection that follows the decode, and
    image_base, the index in the run of the batch's first image (sampling).  Built once per call, checked once, keyed
    once and handed to the one C entry, comic_decoder_beam_search.  cons / grp / smp / trc are the ACTIVE options or None:
    what the executor is given."""
    length_penalty_weight: float = 0.0
    constraints: BeamConstraints | None = None
    groups: BeamGroups | None = None
    sampling: BeamSampling | None = None
    truncation: BeamTruncation | None = None
    required: BeamRequired | None = None
    consensus: Consensus | None = None
    image_base: int = 0
    reward: Reward | None = None
    reward_refs: RewardRefs | None = None
    reward_baseline_ids: object = field(default=None, compare=False, hash=False)     # (an array: no part of the value)
    prefix: BeamPrefix | None = None

    cons = property(lambda self: _active(self.constraints))
    grp = property(lambda self: _active(self.groups))
    smp = property(lambda self: _active(self.sampling))
    trc = property(lambda self: _active(self.truncation))

    @classmethod
    def of(cls, options, **keywords):
        """The one BeamOptions of a beam_search call: `options`, or the option keywords; both is a ValueError."""
        if options is None:
            return cls(**keywords)
        if any(v is not None and not (isinstance(v, (int, float)) and v == 0) for v in keywords.values()):
            raise ValueError('beam_search: give `options` or the option keywords, not both')
        return options

    @property
    def active(self):
        """Whether any executor option is on: the ensemble executor decodes, not Decoder's fast single-member one."""
        return any(x is not None for x in (self.cons, self.grp, self.smp, self.required, self.prefix))

    def check(self, spec, beam, batch, max_steps):
        """Every option's rules and the rules between them, on the host before anything is built or launched."""
        if self.consensus is not None:
            self.consensus.check(beam, max_steps)
        if self.reward is not None:
            if self.reward_refs is None:
                raise ValueError('reward: reward_refs (the RewardRefs of the batch) is missing')
            self.reward.check(beam, max_steps, None if self.reward_baseline_ids is None else self.reward_baseline_ids.shape[0])
        elif self.reward_refs is not None or self.reward_baseline_ids is not None:
            raise ValueError('reward_refs / reward_baseline_ids apply to the reward only: give reward')
        if self.prefix is not None:
            self.prefix.check(spec, beam, batch, max_steps)
        if self.truncation is not None:
            self.truncation.check(self.sampling)
        if self.required is not None:
            self.required.check(spec, beam, batch, max_steps, self.constraints, self.groups, self.sampling)
        if self.groups is not None:
            self.groups.check(beam, spec.V)
        if self.sampling is not None:
            self.sampling.check(beam, self.length_penalty_weight, self.groups)
        if self.cons is not None:
            self.cons.check(spec, beam, max_steps)

    def ctx_key(self):
        """What a captured graph bakes in: the penalty weight, the constraints, the groups, the temperature, top_k / top_p
        (the floats as the fp32 values the kernels see) and (n_words, stride).  Not what is written in front of every launch:
        the seed, image_base and the required table.  None and every inactive option give the plain key."""
        return (float(self.length_penalty_weight),) + tuple(
            None if x is None else key(x) for x, key in (
                (self.cons, BeamConstraints.key), (self.grp, BeamGroups.key), (self.smp, BeamSampling.ctx_key),
                (self.trc, BeamTruncation.ctx_key), (self.required, BeamRequired.ctx_key)))

    def context_key(self):
        """The key of a decode context: ctx_key(), and the prefix's (its width alone) behind it when there is one --
        prefix=None keys the contexts of a decode without one exactly as before."""
        return self.ctx_key() if self.prefix is None else self.ctx_key() + (self.prefix.ctx_key(),)

    def c_record(self, ctx):
        """The comic_beam_options of a decode context.  The structs it points to are kept alive on the context (ctx.cons,
        .grp, .smp, .trc, .rqd: None where the option is off); sampling and required words name the context's device words
        ctx.seed and ctx.req."""
        ctx.cons, ctx.grp, ctx.trc, ctx.rqd = (None if x is None else x.c_struct()
                                               for x in (self.cons, self.grp, self.trc, self.required))
        ctx.smp = None if self.smp is None else self.smp.c_struct(ctx.seed.data_ptr())
        return L.BeamOptions(*[None if x is None else C.addressof(x) for x in (ctx.cons, ctx.grp, ctx.smp, ctx.trc, ctx.rqd)],
                             ctx.req.data_ptr() if self.required is not None else None)


def options_from_config(c, load=True):
    """The BeamOptions a configuration asks for, without the per-batch parts (the required rows, the prefix rows, image_base).
    load=False: the refusals alone, in the order the command line has always raised them, with nothing read that a run
    reads later: no idf table, and no constraints (their words map through the vocabulary of the input manager)."""
    grp, smp, trc = groups_from_config(c), sampling_from_config(c), truncation_from_config(c)
    required_from_config(c)
    prefix_from_config(c)
    cns = consensus_from_config(c, load_idf=load)
    return BeamOptions(getattr(c, 'infer_length_penalty_weight', 0.0) or 0.0, constraints_from_config(c) if load else None,
                       grp, smp, trc, None, cns)


def decode_dir_suffix(c):
    """The directory suffix of a configuration's decode: every option's own, in the order they were added."""
    return (constraints_dir_suffix(c) + groups_dir_suffix(c) + sampling_dir_suffix(c) + truncation_dir_suffix(c)
            + consensus_dir_suffix(c) + required_dir_suffix(c) + prefix_dir_suffix(c))


TEACHER_LDS_BYTES = 160 * 1024          # comic_teacher_topk holds a row of V probabilities + 2048 bytes of scratch in LDS


@dataclass(frozen=True)
class SoftTargets:
    """Soft targets of the XE loss as one immutable value (comic_soft_targets): for a token with target y the loss is the
    cross-entropy H(q, p) against q = (1 - smoothing - teacher_weight) e_y + smoothing / V + teacher_weight q_T, with q_T
    the renormalised top_k entries of a teacher's mean tempered softmax (Decoder.teacher_targets).  H(q, p), not the KL
    divergence: they differ by the entropy of q, a constant in the parameters.  The student's temperature is 1 (no
    temperature^2 factor); `temperature` is the teacher's.  Checked at construction."""
    smoothing: float = 0.0
    teacher_weight: float = 0.0
    top_k: int = 16
    temperature: float = 1.0

    def __post_init__(self):
        e, w = self.smoothing, self.teacher_weight
        for name, x in (('smoothing', e), ('teacher_weight', w), ('temperature', self.temperature)):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x):
                raise ValueError('SoftTargets: %s must be a number, got %r' % (name, x))
        if not 0.0 <= e < 1.0:
            raise ValueError('SoftTargets: smoothing must be in [0, 1), got %r' % (e,))
        if not 0.0 <= w <= 1.0:
            raise ValueError('SoftTargets: teacher_weight must be in [0, 1], got %r' % (w,))
        if e + w > 1.0:
            raise ValueError('SoftTargets: smoothing + teacher_weight must not exceed 1, got %r' % (e + w,))
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, int) or not 1 <= self.top_k <= L.SOFT_MAX_K:
            raise ValueError('SoftTargets: top_k must be an integer in [1, %d], got %r' % (L.SOFT_MAX_K, self.top_k))
        if not 0.0 < self.temperature < math.inf:
            raise ValueError('SoftTargets: temperature must be in (0, inf), got %r' % (self.temperature,))

    @property
    def active(self):
        return self.smoothing > 0.0 or self.teacher_weight > 0.0

    @property
    def distils(self):
        return self.teacher_weight > 0.0

    def ctx_key(self):
        """What a captured training graph bakes in: the two weights as the fp32 values the kernel sees, and K when a table
        is read.  Not the table's contents (copied in front of every launch) nor the teacher's temperature."""
        return (float(np.float32(self.smoothing)), float(np.float32(self.teacher_weight)),
                self.top_k if self.distils else 0)

    def check_vocabulary(self, V):
        if self.distils and self.top_k > V:
            raise ValueError('SoftTargets: top_k %d exceeds the vocabulary size %d' % (self.top_k, V))


def soft_targets_from_config(c):
    """The SoftTargets a configuration asks for (label_smoothing, distill_*), or None when every field is at its default."""
    eps = float(getattr(c, 'label_smoothing', 0.0) or 0.0)
    lam = float(getattr(c, 'distill_weight', 0.0) or 0.0) if getattr(c, 'distill_checkpoints', None) else 0.0
    if eps == 0.0 and lam == 0.0:
        return None
    k, tau = getattr(c, 'distill_top_k', None), getattr(c, 'distill_temperature', None)
    return SoftTargets(eps, lam, 16 if k is None else int(k), 1.0 if tau is None else float(tau))


def teacher_table(members, weights, fm, im_embed, captions, top_k, temperature):
    """ids, probs [T,B,K] of the members' weighted mean tempered softmax (comic_teacher_topk): every member runs the
    forward-only phase of its own executor on the same features and captions, then ONE launch covers their logits.
    Nothing is synchronised; the tables are persistent per shape on the first member (valid until its next call)."""
    first = members[0]
    torch, V = first.torch, first.spec.V
    SoftTargets(0.0, 1.0, top_k, temperature).check_vocabulary(V)          # K and the temperature, before any launch
    if V * 4 + 2048 > TEACHER_LDS_BYTES:
        raise ValueError('teacher_targets: a row of V = %d probabilities does not fit the %d bytes of LDS (V <= %d)'
                         % (V, TEACHER_LDS_BYTES, (TEACHER_LDS_BYTES - 2048) // 4))
    ctxs = [m._forward_logits(fm, im_embed, captions) for m in members]
    B, T, Tp = ctxs[0].key[:3]
    tab = first._teacher_tabs.get((B, T, top_k))
    if tab is None:
        tab = first._teacher_tabs[(B, T, top_k)] = (torch.zeros((T, B, top_k), dtype=torch.int32, device=first.device),
                                     torch.zeros((T, B, top_k), dtype=torch.float32, device=first.device))
    n = len(members)
    ptrs = (C.c_void_p * n)(*[c.logits.data_ptr() for c in ctxs])
    w = (C.c_float * n)(*weights)
    L.check(first.lib.comic_teacher_topk(ptrs, w, n, ctxs[0].stage.ptr['lens'], B, T, Tp, V, float(temperature),
                                         int(top_k), tab[0].data_ptr(), tab[1].data_ptr(), L.stream_ptr()), 'teacher_topk')
    return tab


def process_inputs(captions, token_type):
    """ModelBase._process_inputs (model_base.py:501-528) on the host.
    -> inputs [B,T] int32, targets [B,T] int32, masks [B,T] fp32, lens [B] int32."""
    sent = np.asarray(captions, np.int64)
    masks = np.sign((sent[:, 1:] + 1).astype(np.float32))
    lens = masks.sum(axis=1).astype(np.int32)
    if token_type == 'word':
        sent = np.maximum(sent, 0)
        inputs = sent[:, :-1]
    else:
        inputs = sent[:, :-1]
        sent = np.maximum(sent, 0)
    targets = sent[:, 1:]
    return (np.ascontiguousarray(inputs, np.int32), np.ascontiguousarray(targets, np.int32),
            np.ascontiguousarray(masks, np.float32), lens)


DEVICE_REWARDS = 'device'               # loss_coefficients(rewards=): comic_scst_coefficients forms them on the stream


def loss_coefficients(wmask, rewards, xe_denom, B):
    """coef, rs [B,T] float32 of the sequence loss (model_base.py:337-347) from the mask: the per-token coefficient the
    kernels multiply the cross-entropy by, and the row scale of the loss reduction.  rewards None: XE, normalised by
    sum(w) + 1e-12 or by `xe_denom`; a host array [B]: SCST, mean_b(xent_b * reward_b); DEVICE_REWARDS: zeros, which the
    device overwrites.  Float32 operations in this order: comic_scst_coefficients repeats them bit for bit."""
    T = wmask.shape[1]
    if rewards is DEVICE_REWARDS:
        rs = coef = np.zeros((B, T), np.float32)
    elif rewards is None:
        den_xe = np.float32(xe_denom) if xe_denom is not None else np.float32(wmask.sum() + np.float32(1e-12))
        rs = np.full((B, T), np.float32(1.0) / den_xe, np.float32)
        coef = wmask / den_xe
    else:
        den = wmask.sum(axis=1, keepdims=True) + np.float32(1e-12)
        rb = (np.asarray(rewards, np.float32)[:, None] / np.float32(B))
        rs = np.broadcast_to(rb / den, (B, T)).astype(np.float32)
        coef = wmask / den * rb
    return coef, rs


def train_stage_fields(B, T):
    """ONE staging block per training step: [seed int64 | inputs, targets, lens int32 | wmask, coef, row scale fp32]."""
    return (('seed', 'int64', (1,)), ('inputs', 'int32', (B, T)), ('targets', 'int32', (B, T)), ('lens', 'int32', (B,)),
            ('wmask', 'float32', (B, T)), ('coef', 'float32', (B, T)), ('row_scale', 'float32', (B, T)))


def score_stage_fields(B, T):
    """ONE staging block per scoring call: [inputs, targets, lens int32 | wmask fp32]."""
    return train_stage_fields(B, T)[1:5]


def staging_layout(fields):
    """Byte offset of every field (name, dtype, shape) of a staging block, and the block's size: the fields follow each
    other in order, and where the dtype changes the offset is rounded up to 8 bytes.  Pure: no GPU, no torch."""
    offsets, at, last = {}, 0, None
    for name, dtype, shape in fields:
        if last is not None and dtype != last:
            at = (at + 7) // 8 * 8
        offsets[name], last = at, dtype
        at += np.dtype(dtype).itemsize * int(np.prod(shape))
    return offsets, at


class Staging:
    """The small host-written operands of a step as one device block, fed by ONE copy from pinned memory.  Two pinned slots
    are used alternately: the host may run ahead of the GPU, and an async H2D copy reads its pinned source when the STREAM
    gets there, so a slot is rewritten only after the copy that last used it has executed (an event per slot).
    dev[name] / ptr[name]: the field's device view / address; every view, device or host, is flat (the kernels' view)."""

    def __init__(self, torch, device, fields):
        self.torch = torch
        offsets, self.nbytes = staging_layout(fields)

        def views(buf):
            return {name: buf[offsets[name]:offsets[name] + np.dtype(dtype).itemsize * int(np.prod(shape))]
                    .view(getattr(torch, dtype)) for name, dtype, shape in fields}
        self.buf = torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        self.dev = views(self.buf)
        self.ptr = {name: t.data_ptr() for name, t in self.dev.items()}
        self._slots = []
        for _ in range(2):
            buf = torch.zeros(self.nbytes, dtype=torch.uint8).pin_memory()
            self._slots.append((buf, {name: t.numpy() for name, t in views(buf).items()}, torch.cuda.Event()))
        self._taken = -1                # slots taken so far - 1: its own counter, nobody else's

    def next_slot(self):
        """Take the next slot, once the copy that last read it has executed -> its host views (numpy, by name)."""
        self._taken += 1
        return self.last_slot()

    def last_slot(self):
        """The slot the last upload used, once that copy has executed -> its host views: a second upload of one step."""
        _, host, copied = self._slots[self._taken % 2]
        copied.synchronize()            # (returns at once on an event that was never recorded)
        return host

    def upload(self):
        """The taken slot to the device block on the current stream, and the slot's event behind the copy."""
        buf, _, copied = self._slots[self._taken % 2]
        self.buf.copy_(buf, non_blocking=True)
        copied.record(self.torch.cuda.current_stream())

    def send(self, fields, again=False):
        """`fields` (arrays or numbers by name) into the next slot -- again=True: into the slot the last upload used, whose
        other fields stand -- and that slot to the device."""
        host = self.last_slot() if again else self.next_slot()
        for name, value in fields.items():
            host[name][:] = np.reshape(value, -1)
        self.upload()


class GraphRunner:
    """Eager or hipGraph execution of a context's launches: run(what, launch, use_graph) calls launch() eagerly; with
    use_graph the second use of `what` on this context captures it and every later one replays the graph.  Uses count
    whether or not they asked for a graph.  what: None for the context's whole launch sequence, 'fwd' / 'bwd' for the
    halves of a split training step; each has its own counter and its own graph."""

    def __init__(self, torch):
        self.torch, self.uses, self.graphs = torch, {}, {}

    def run(self, what, launch, use_graph):
        torch = self.torch
        self.uses[what] = used = self.uses.get(what, 0) + 1
        graph = self.graphs.get(what)
        if use_graph and graph is None and used >= 2:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                launch()
            self.graphs[what] = graph
        if use_graph and graph is not None:
            graph.replay()
        else:
            launch()


class _Context:
    """Persistent buffers of one shape of one entry point, with the graphs of its launches.  The constructors
    (Decoder._train_ctx, _score_ctx, _infer_ctx, EnsembleDecoder._ctx) add the buffers every use needs; what is set later,
    or only for some uses, is declared in the subclasses."""

    def __init__(self, torch, key):
        self.key, self.runner = key, GraphRunner(torch)

    @property
    def graph(self):
        """The graph of the whole step / scoring call / decode loop, or None before its capture."""
        return self.runner.graphs.get(None)


class _StepContext(_Context):
    """A training or scoring context."""
    stage = None                        # the Staging block
    masks = None                        # training: the dropout masks by name (views of mask_buf)
    soft = None                         # training with soft targets: the comic_soft_targets record
    fm_in = im_in = None                # what the step reads: the caller's tensors in place, or the context's copies
    split_open = False                  # a phase='fwd' call waits for its phase='bwd'
    inject_timeout = False              # the next eager step runs with COMIC_DEC_INJECT_TIMEOUT (tests)


class _DecodeContext(_Context):
    """A greedy / beam / ensemble decode context."""
    ids_host = eos_host = None          # greedy(defer=True): pinned copies of ids and first_eos
    pred = pred_host = steps_host = None    # beam_search_ids: the gathered ids, pinned copies of them and of steps
    fetched = None                      # the event behind those copies
    keep = None                         # a temporary the enqueued launches still read
    seed = req = None                   # sampling / required words: device words written in front of every launch
    prefix = pfx = None                 # forced prefix: the comic_beam_prefix record and the device table
    cons = grp = smp = trc = rqd = None     # the C structs of the active options, kept alive (BeamOptions.c_record)


class Decoder:
    """Device decoder: parameters, gradients and native step calls."""

    def __init__(self, spec: DecoderSpec, params: dict | None = None, device='cuda:0', seed=0):
        import torch
        self.torch = torch
        self.lib = L.load()
        self.spec, self.device = spec, device
        self.params = FlatParams(spec.param_shapes(), device, status_tail=True)
        self.params.load(params if params is not None else init_params(spec, seed))
        self.grads = self.params.like()
        self._ws = None
        self._ws_bytes = 0
        self._dropout_calls = 0
        self.set_dropout_stream(seed, 0)
        self._ctx, self._score_ctxs, self._infer_ctxs, self._teacher_tabs = {}, {}, {}, {}

    # ------------------------------------------------------------------ helpers --------
    def _workspace(self, nbytes):
        if self._ws is None or self._ws_bytes < nbytes:
            self._ws = self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)
            self._ws_bytes = int(nbytes)
        return self._ws

    def _dev(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=False)

    def make_masks(self, B, Tp, seed):
        """Bernoulli keep masks generated on the device (counter-based; TF's RNG stream is
        not reproducible, SURVEY §7 'Dropout parity')."""
        torch, s = self.torch, self.spec
        EA = s.E + s.A
        out = {}
        off = 0
        for name, shape, keep in (('init_in', (B, EA), 1 - s.dropout_rnn_in), ('inp', (Tp, B, EA), 1 - s.dropout_rnn_in),
                                  ('out', (Tp, B, s.D), 1 - s.dropout_rnn_out),
                                  ('alpha', (Tp, B, s.H, s.M), s.attn_keep_prob)):
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            L.check(self.lib.comic_dropout_mask(t.data_ptr(), t.numel(), keep, int(seed), off, L.stream_ptr()),
                    'dropout_mask')
            off += t.numel()
            out[name] = t
        return out

    # ------------------------------------------------------------------ training -------
    def _train_ctx(self, B, T, Tp, training, gen_masks, want_input_grads, soft=None):
        """Persistent device buffers (+ hipGraph) of one training-step shape; `soft` (an active SoftTargets) keys a context
        of its own, whose graph holds the record's scalars."""
        key = (B, T, Tp, bool(training), bool(gen_masks), bool(want_input_grads))
        if soft is not None:
            key += (soft.ctx_key(),)
        ctx = self._ctx.get(key)
        if ctx is not None:
            return ctx
        torch, s, dev = self.torch, self.spec, self.device
        ctx = _StepContext(torch, key)
        f32 = dict(dtype=torch.float32, device=dev)
        ctx.stage = Staging(torch, dev, train_stage_fields(B, T))
        ctx.fm = torch.empty((B, s.M, s.C), **f32)
        ctx.im = torch.empty((B, s.Cg), **f32)
        EA = s.E + s.A
        if training:
            # one buffer, four views (generated by ONE launch: comic_dropout_masks4_dev)
            shapes = dict(init_in=(B, EA), inp=(Tp, B, EA), out=(Tp, B, s.D), alpha=(Tp, B, s.H, s.M))
            sizes = [int(np.prod(v)) for v in shapes.values()]
            ctx.mask_buf = torch.empty(sum(sizes), **f32)
            ctx.masks, off = {}, 0
            for (k, shp), n in zip(shapes.items(), sizes):
                ctx.masks[k] = ctx.mask_buf[off:off + n].view(shp)
                off += n
            ctx.mask_n4 = (C.c_int64 * 4)(*sizes)
            ctx.mask_keep4 = (C.c_float * 4)(1 - s.dropout_rnn_in, 1 - s.dropout_rnn_in, 1 - s.dropout_rnn_out,
                                             s.attn_keep_prob)
        ctx.logits = torch.empty((T, B, s.V), **f32)
        ctx.ids = torch.empty((T, B), dtype=torch.int32, device=dev)
        ctx.hist = torch.empty((Tp, B, s.H, s.M), **f32)
        ctx.loss_rows = torch.empty(T * B, **f32)
        ctx.map_loss = torch.zeros(1, **f32)
        ctx.loss = torch.zeros(1, **f32)
        ctx.dfm = torch.empty((B, s.M, s.C), **f32) if want_input_grads else None
        ctx.dim = torch.empty((B, s.Cg), **f32) if want_input_grads else None
        ctx.desc = s.desc(training)
        ctx.nbytes = self.lib.comic_decoder_train_workspace(C.byref(ctx.desc), B, T)
        ctx.ws = torch.empty(int(ctx.nbytes), dtype=torch.uint8, device=dev)
        if soft is not None:    # the record, the hard-loss rows and the step's own copy of the teacher's table
            K = soft.top_k
            ctx.nll_rows = torch.zeros(T * B, **f32)
            ctx.nll = torch.zeros(1, **f32)
            ctx.t_ids = torch.zeros((T, B, K), dtype=torch.int32, device=dev) if soft.distils else None
            ctx.t_probs = torch.zeros((T, B, K), **f32) if soft.distils else None
            ctx.soft = L.SoftTargets(soft.smoothing, soft.teacher_weight, K if soft.distils else 0, L.ptr(ctx.t_ids),
                                     L.ptr(ctx.t_probs), ctx.nll_rows.data_ptr())
        self._ctx[key] = ctx
        return ctx

    def _stage_teacher(self, ctx, soft, teacher):
        """The teacher's table of this step into the context's own (a captured graph holds addresses), on the stream."""
        if soft is None or not soft.distils:
            return
        torch = self.torch
        if teacher is None:
            raise ValueError('train_step: teacher_weight %g without a teacher table (teacher=(ids, probs))'
                             % soft.teacher_weight)
        ids, probs = teacher
        want = tuple(ctx.t_ids.shape)
        if (not torch.is_tensor(ids) or not torch.is_tensor(probs) or tuple(ids.shape) != want or tuple(probs.shape) != want
                or ids.dtype != torch.int32 or probs.dtype != torch.float32 or not ids.is_cuda or not probs.is_cuda):
            raise ValueError('train_step: teacher must be device tensors (ids int32, probs float32) of shape [T, B, K] = %r'
                             % (want,))
        ctx.t_ids.copy_(ids)
        ctx.t_probs.copy_(probs)

    def voided_steps(self):
        """Training steps the device voided so far (a bounded wait of a persistent loop expired: NaN loss, no update;
        comic_decoder_params::status of the parameter table).  Synchronises: for log points, not for every step."""
        return int(float(self.params.status))

    def set_dropout_stream(self, seed, rank=0):
        """Base of the per-step dropout seeds: a function of the run's seed (tf.set_random_seed(rand_seed), train_fn.py:35)
        and of the data-parallel rank, so that runs 1/2/3 and the ranks of one run draw different masks."""
        x = (int(seed) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15 + (int(rank) + 1) * 0xBF58476D1CE4E5B9
        x ^= x >> 31
        self._dropout_base = (x * 0x94D049BB133111EB) & 0x3FFFFFFFFFFFFFFF

    def _train_device(self, ctx, phase=None):
        """Device-only part of a training step (no host sync, no host memcpy): capturable.
        phase 'fwd' / 'bwd': the forward to the logits / the loss and the backward (COMIC_DEC_PHASE_*)."""
        torch, s = self.torch, self.spec
        B, T, Tp, training, gen_masks = ctx.key[:5]
        st = L.stream_ptr()
        m = ctx.masks or {}
        if training and gen_masks and phase != 'bwd':
            L.check(self.lib.comic_dropout_masks4_dev(ctx.mask_buf.data_ptr(), ctx.mask_n4, ctx.mask_keep4,
                                                      ctx.stage.ptr['seed'], st), 'dropout_masks4')
            if s.recurrent_dropout:
                # variational recurrent dropout (model_base.py:645; [TF-1.9] DropoutWrapper draws its input / output
                # noise once per run with a batch dimension of 1): the first row of the drawn masks serves every batch
                # row and time step, the init call through the same wrapper included; the attention dropout is not
                # part of the wrapper and stays per step
                row_in = m['inp'][0, 0].clone()
                row_out = m['out'][0, 0].clone()
                m['inp'].copy_(row_in.expand_as(m['inp']))
                m['init_in'].copy_(row_in.expand_as(m['init_in']))
                m['out'].copy_(row_out.expand_as(m['out']))
        at = ctx.stage.ptr
        ptab, gtab = self.params.table(), self.grads.table()
        inject, ctx.inject_timeout = ctx.inject_timeout, False
        ctx.desc.flags = (L.decoder_flags_from_env() | {None: 0, 'fwd': L.DEC_PHASE_FWD, 'bwd': L.DEC_PHASE_BWD}[phase]
                          | (L.DEC_INJECT_TIMEOUT if inject else 0))
        args = (C.byref(ctx.desc), C.byref(ptab), C.byref(gtab), ctx.fm_in.data_ptr(), ctx.im_in.data_ptr(),
                at['inputs'], at['targets'], at['wmask'], at['coef'], at['lens'], B, T, Tp,
                L.ptr(m.get('init_in')), L.ptr(m.get('inp')), L.ptr(m.get('out')), L.ptr(m.get('alpha')),
                ctx.logits.data_ptr(), ctx.ids.data_ptr(), ctx.hist.data_ptr(), ctx.loss_rows.data_ptr(),
                ctx.map_loss.data_ptr(), L.ptr(ctx.dfm), L.ptr(ctx.dim), ctx.ws.data_ptr(), ctx.nbytes, st)
        if ctx.soft is None:
            L.check(self.lib.comic_decoder_train_step(*args), 'decoder_train_step')
        else:
            L.check(self.lib.comic_decoder_train_step_soft(*args, C.byref(ctx.soft)), 'decoder_train_step_soft')
        if phase == 'fwd':
            return
        # sequence_loss reduction (model_base.py:337-347): rows carry xent*w; rs = 1/denominator (* reward/B)
        L.check(self.lib.comic_weighted_sum_tb(ctx.loss_rows.data_ptr(), at['row_scale'], T, B,
                                               ctx.loss.data_ptr(), st), 'weighted_sum_tb')
        if ctx.soft is not None:            # the hard loss beside the optimised one, by the same reduction
            L.check(self.lib.comic_weighted_sum_tb(ctx.nll_rows.data_ptr(), at['row_scale'], T, B,
                                                   ctx.nll.data_ptr(), st), 'weighted_sum_tb')

    def train_step(self, fm, im_embed, captions, masks=None, rewards=None, training=True, seed=None,
                   want_input_grads=False, xe_denom=None, use_graph=False, on_inputs_consumed=None, dp=None,
                   copy_inputs=True, phase=None, inject_timeout=False, soft=None, teacher=None):
        """One teacher-forced forward + backward.  `captions` [B,L] int (PAD = -1).
        phase: None = the whole step.  'fwd' = everything no loss coefficient enters (forward to the logits; `rewards` is
        ignored) and 'bwd' = the rest, with the SAME captions and now the rewards: the SCST step enqueues 'fwd' as soon as
        the rollouts are back and scores them on the host while it runs (the same kernels in the same order: same bits).
        masks: None -> generated on device when training; dict(init_in, inp, out, alpha) of
        device tensors or numpy arrays -> injected (parity tests).  rewards [B] -> SCST loss
        mean_b(xent_b * reward_b) (model_base.py:342-347).  rewards as a float32 DEVICE tensor [B] (the advantage of
        Decoder.scst_reward): the loss coefficients are formed on the stream by comic_scst_coefficients with the float32
        operations of the host formula -- same bits, no host copy of them and no synchronisation; the tensor must stay
        unchanged until the step has executed.
        xe_denom: override of the XE normaliser sum(w)+1e-12 (data parallel: global token count / world size,
        so that the rank-mean of the gradients equals the single-process gradient of the global batch).
        dp: a trainer.DataParallel with world > 1 -> the same normaliser formed ON THE DEVICE: the token count of
        this rank's batch is summed from the staged mask, all-reduced on the stream, and the per-token coefficients
        the kernels read are rescaled in place -- no host synchronisation in the step.
        copy_inputs=False: the step reads `fm` / `im_embed` in place instead of from its own copies (13 MB less
        device-to-device traffic per step at batch 64).  The caller then keeps both tensors unchanged until the step has
        EXECUTED (stream order: anything it enqueues on this stream afterwards is safe) and `on_inputs_consumed` is
        called after the step's launches rather than before them.  Ignored with use_graph (a graph holds addresses).
        use_graph: replay the step from a hipGraph captured per (B, T, T') shape (the second call with
        a shape captures it) -- removes the ~450 host launches of a step from the critical path.
        soft: a SoftTargets -> the loss is the cross-entropy against its soft targets (label smoothing, and with
        teacher_weight > 0 the `teacher` table (ids, probs), device tensors [T,B,K] of teacher_targets); one launch of the
        step changes (csrc/xent_soft.hip), `loss` is the optimised soft loss and `nll` the hard one.  None, an inactive
        record or training=False: the step of always.  With `rewards` a ValueError: soft targets are XE training.
        Returns dict(loss, nll, map_loss, logits [B,T,V], ids [B,T], attn_maps [B,H,T',M]) (device views
        of persistent buffers: valid until the next call with the same shape)."""
        soft = self._checked_soft(soft, training, rewards, teacher, phase)
        inputs, targets, wmask, lens = process_inputs(captions, self.spec.token_type)
        B, T = inputs.shape
        Tp = int(lens.max())
        dev_rewards = self._checked_device_rewards(rewards, B)
        coef, rs = loss_coefficients(wmask, rewards if dev_rewards is None else DEVICE_REWARDS, xe_denom, B)
        gen_masks = bool(training and masks is None)
        use_masks = bool(training or masks is not None)
        ctx = self._train_ctx(B, T, Tp, use_masks, gen_masks, want_input_grads, soft)
        if phase != 'fwd':
            self._stage_teacher(ctx, soft, teacher)
        if phase == 'bwd':          # second call of a split step: only the coefficients are new
            assert ctx.split_open, 'train_step(phase="bwd") without its phase="fwd" call'
            ctx.split_open = False
            if dev_rewards is not None:                           # the mask is on the device since the forward call
                self._device_coefficients(ctx, dev_rewards)
            else:                                                 # into the slot its forward call staged: same inputs
                ctx.stage.send(dict(coef=coef, row_scale=rs), again=True)
            ctx.runner.run('bwd', lambda: self._train_device(ctx, 'bwd'), use_graph)
            return self._train_result(ctx, Tp)
        fields = dict(inputs=inputs, targets=targets, lens=lens, wmask=wmask, coef=coef, row_scale=rs)
        if gen_masks:
            fields['seed'] = self._dropout_seed(seed)
        ctx.stage.send(fields)
        if dev_rewards is not None and phase != 'fwd':
            self._device_coefficients(ctx, dev_rewards)
        if masks is not None:
            self._inject_masks(ctx, masks)
        if dp is not None and dp.world > 1 and rewards is None:
            self._rescale_data_parallel(ctx, dp)
        direct = self._bind_inputs(ctx, fm, im_embed, not copy_inputs and not use_graph, on_inputs_consumed)
        if phase == 'fwd':
            ctx.split_open = True
        if inject_timeout:          # fault injection of THIS call (COMIC_DEC_INJECT_TIMEOUT, tests): eager launches only
            assert not use_graph and phase is None
            ctx.inject_timeout = True
        ctx.runner.run(phase, lambda: self._train_device(ctx, phase), use_graph)
        if direct and on_inputs_consumed is not None:   # stream order: whatever the caller enqueues now runs after the step
            on_inputs_consumed()
        return None if phase == 'fwd' else self._train_result(ctx, Tp)

    def _checked_soft(self, soft, training, rewards, teacher, phase):
        """The active SoftTargets of a train_step call or None, refused where they do not apply."""
        soft = _active(soft) if training else None
        if soft is not None:
            if rewards is not None:
                raise ValueError('train_step: soft targets and SCST rewards do not combine')
            soft.check_vocabulary(self.spec.V)
            if soft.distils and teacher is None and phase != 'fwd':
                raise ValueError('train_step: teacher_weight %g without a teacher table (teacher=(ids, probs))'
                                 % soft.teacher_weight)
        return soft

    def _checked_device_rewards(self, rewards, B):
        """`rewards` where it is a device tensor (else None): float32 [B], contiguous.  comic_scst_coefficients then forms
        coef / rs on the stream from the staged mask, into the device staging block; the host writes neither."""
        torch = self.torch
        if not torch.is_tensor(rewards):
            return None
        if tuple(rewards.shape) != (B,) or rewards.dtype != torch.float32 or not rewards.is_cuda:
            raise ValueError('train_step: device rewards must be a float32 device tensor [%d], got %s %r'
                             % (B, rewards.dtype, tuple(rewards.shape)))
        return rewards.contiguous()

    def _dropout_seed(self, seed):
        """The seed of a step's device-generated masks: the caller's, or the next of this decoder's stream."""
        if seed is None:
            self._dropout_calls += 1
            seed = (self._dropout_base + self._dropout_calls) & 0x7FFFFFFFFFFFFFFF
        return int(seed)

    def _inject_masks(self, ctx, masks):
        """Given dropout masks (device tensors or numpy arrays) into the context's own, on the stream."""
        torch = self.torch
        for k, v in masks.items():
            ctx.masks[k].copy_(v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float32)))

    def _rescale_data_parallel(self, ctx, dp):
        """coef and the row scale of the device staging block from the GLOBAL token count (train_step's dp=): formed on
        the stream behind the staging copy, no host synchronisation."""
        d = ctx.stage.dev
        inv = 1.0 / dp.global_xe_denominator(d['wmask'])
        self.torch.mul(d['wmask'], inv, out=d['coef'])
        d['row_scale'][:] = inv

    def _bind_inputs(self, ctx, fm, im_embed, in_place, on_inputs_consumed):
        """ctx.fm_in / .im_in, what the step reads: the caller's tensors (in_place, where they are contiguous: -> True, and
        the caller is told after the step's launches) or the context's copies, after which the caller's may be overwritten."""
        torch, s = self.torch, self.spec
        B = ctx.key[0]
        assert fm.shape == (B, s.M, s.C) and im_embed.shape == (B, s.Cg), (fm.shape, im_embed.shape)
        assert fm.dtype == torch.float32 and im_embed.dtype == torch.float32
        if in_place and fm.is_contiguous() and im_embed.is_contiguous():
            ctx.fm_in, ctx.im_in = fm, im_embed
            return True
        ctx.fm.copy_(fm)
        ctx.im.copy_(im_embed)
        ctx.fm_in, ctx.im_in = ctx.fm, ctx.im
        if on_inputs_consumed is not None:      # the encoder buffers may be overwritten from here on
            on_inputs_consumed()
        return False

    @staticmethod
    def _train_result(ctx, Tp):
        return dict(loss=ctx.loss[0], nll=(ctx.loss if ctx.soft is None else ctx.nll)[0], map_loss=ctx.map_loss[0],
                    logits=ctx.logits.permute(1, 0, 2), ids=ctx.ids.t(), attn_maps=ctx.hist.permute(1, 2, 0, 3),
                    dfm=ctx.dfm, dim_embed=ctx.dim, Tp=Tp)

    def _forward_logits(self, fm, im_embed, captions):
        """The forward-only phase of this decoder's executor without dropout (phase='fwd', training=False, the call the
        SCST step makes): -> the context whose .logits [T,B,V] hold rows t < T' and whose staging block holds lens."""
        self.train_step(fm, im_embed, captions, training=False, phase='fwd')
        inputs, _, _, lens = process_inputs(captions, self.spec.token_type)
        return self._train_ctx(inputs.shape[0], inputs.shape[1], int(lens.max()), False, False, False)

    def teacher_targets(self, fm, im_embed, captions, top_k=16, temperature=1.0):
        """This decoder as a teacher: ids, probs [T,B,top_k] (int32, float32 device tensors) of its tempered softmax on the
        captions' teacher-forced rows, for train_step(soft=, teacher=) of a student (teacher_table)."""
        return teacher_table([self], [1.0], fm, im_embed, captions, top_k, temperature)

    def _device_coefficients(self, ctx, rewards):
        """coef and rs of the device staging block from its mask and the device rewards [B] (comic_scst_coefficients):
        stream-ordered behind the staging copy, in front of the step that reads them."""
        B, T = ctx.key[:2]
        at = ctx.stage.ptr
        L.check(self.lib.comic_scst_coefficients(at['wmask'], rewards.data_ptr(), B, T, at['coef'], at['row_scale'],
                                                 L.stream_ptr()), 'scst_coefficients')

    # ------------------------------------------------------------------ scoring --------
    def _score_ctx(self, B, T, Tp, want_attention):
        """Persistent device buffers (+ hipGraph) of one scoring shape: a context and staging slots of their own, so a
        scoring call between two training steps of the same shape disturbs neither."""
        key = (B, T, Tp, bool(want_attention))
        ctx = self._score_ctxs.get(key)
        if ctx is not None:
            return ctx
        torch, s, dev = self.torch, self.spec, self.device
        ctx = _StepContext(torch, key)
        f32 = dict(dtype=torch.float32, device=dev)
        ctx.stage = Staging(torch, dev, score_stage_fields(B, T))
        ctx.wmask = ctx.stage.dev['wmask']
        ctx.fm = torch.empty((B, s.M, s.C), **f32)
        ctx.im = torch.empty((B, s.Cg), **f32)
        ctx.token_logp = torch.zeros((T, B), **f32)
        ctx.logp = torch.zeros(B, **f32)
        ctx.hist = torch.empty((Tp, B, s.H, s.M), **f32) if want_attention else None
        ctx.desc = s.desc(False)
        ctx.nbytes = self.lib.comic_decoder_score_workspace(C.byref(ctx.desc), B, T)
        assert ctx.nbytes > 0, 'comic_decoder_score_workspace failed'
        ctx.ws = torch.empty(int(ctx.nbytes), dtype=torch.uint8, device=dev)
        self._score_ctxs[key] = ctx
        return ctx

    def _score_device(self, ctx):
        """Device-only part of a scoring call (no host sync, no host memcpy): capturable."""
        B, T, Tp, _ = ctx.key
        at = ctx.stage.ptr
        ptab = self.params.table()
        ctx.desc.flags = L.decoder_flags_from_env()
        L.check(self.lib.comic_decoder_score(
            C.byref(ctx.desc), C.byref(ptab), ctx.fm.data_ptr(), ctx.im.data_ptr(), at['inputs'], at['targets'],
            at['wmask'], at['lens'], B, T, Tp,
            ctx.token_logp.data_ptr(), ctx.logp.data_ptr(), L.ptr(ctx.hist), ctx.ws.data_ptr(), ctx.nbytes,
            L.stream_ptr()), 'decoder_score')

    def score(self, fm, im_embed, captions, want_attention=False, use_graph=False):
        """Teacher-forced log-likelihoods of given captions, forward only (comic_decoder_score): no dropout, no gradient,
        no logits tensor at a large vocabulary.  `captions` [B,L] int (PAD = -1), processed as in train_step.
        use_graph: replay from a hipGraph captured per (B, T, T') shape (the second call with a shape captures it).
        Returns dict(token_log_probs [B,T] (0 at padding), log_prob [B] (their float32 sum in t order), lengths [B],
        attn_maps [B,H,T',M] or None): device views of persistent buffers, valid until the next call with the shape."""
        torch, s = self.torch, self.spec
        inputs, targets, wmask, lens = process_inputs(captions, s.token_type)
        B, T = inputs.shape
        Tp = int(lens.max())
        assert Tp > 0, 'score: every caption is empty'
        ctx = self._score_ctx(B, T, Tp, want_attention)
        ctx.stage.send(dict(inputs=inputs, targets=targets, lens=lens, wmask=wmask))
        assert fm.shape == (B, s.M, s.C) and im_embed.shape == (B, s.Cg), (fm.shape, im_embed.shape)
        assert fm.dtype == torch.float32 and im_embed.dtype == torch.float32
        ctx.fm.copy_(fm)
        ctx.im.copy_(im_embed)
        ctx.runner.run(None, lambda: self._score_device(ctx), use_graph)
        return dict(token_log_probs=ctx.token_logp.t(), log_prob=ctx.logp, lengths=torch.from_numpy(lens.copy()),
                    attn_maps=ctx.hist.permute(1, 2, 0, 3) if ctx.hist is not None else None, Tp=Tp, wmask=ctx.wmask)

    # ------------------------------------------------------------------ decoding -------
    def max_iterations(self, infer_max_length, vocab_len):
        """model_base.py:708-714."""
        it = infer_max_length
        if self.spec.token_type == 'radix':
            it *= len(number_to_base(vocab_len, self.spec.start_id))    # start_id == radix_base
        elif self.spec.token_type == 'char':
            it *= 5
        return it

    def _infer_ctx(self, kind, B, W, max_steps, want_logits, fm, im_embed, slot=0):
        """Persistent buffers (+ a hipGraph of the whole decode loop, captured on the second call
        with the same shape) of greedy / beam decoding: the executors run all `max_steps` steps on
        the device without host synchronisation, so one graph launch replaces ~8 kernel launches
        per step of host work."""
        torch, s = self.torch, self.spec
        key = (kind, B, W, max_steps, bool(want_logits), int(slot))      # slot: independent buffer sets (decodes in flight on several streams)
        ctx = self._infer_ctxs.get(key)
        if ctx is None:
            ctx = _DecodeContext(torch, key)
            R = B * W
            i32 = dict(dtype=torch.int32, device=self.device)
            f32 = dict(dtype=torch.float32, device=self.device)
            ctx.fm = torch.empty((B, s.M, s.C), **f32)
            ctx.im = torch.empty((B, s.Cg), **f32)
            ctx.hist = torch.empty((max_steps, R, s.H * s.M), **f32)
            if kind == 'greedy':
                ctx.ids = torch.empty((max_steps, B), **i32)
                ctx.logits = torch.empty((max_steps, B, s.V), **f32) if want_logits else None
                ctx.first_eos = torch.empty(B, **i32)
            else:
                _beam_outputs(ctx, torch, self.device, B, W, max_steps)
            ctx.desc = s.desc(False)
            ctx.nbytes = int(self.lib.comic_decoder_infer_workspace(C.byref(ctx.desc), R, max_steps))
            ctx.ws = torch.empty(ctx.nbytes, dtype=torch.uint8, device=self.device)   # own workspace: graph-stable
            ctx.ptab = self.params.table()
            self._infer_ctxs[key] = ctx
        ctx.fm.copy_(fm.reshape(ctx.fm.shape))
        ctx.im.copy_(im_embed.reshape(ctx.im.shape))
        return ctx

    def greedy(self, fm, im_embed, max_steps, want_logits=False, use_graph=True, defer=False):
        """rnn_decoder_search(greedy) (ops_rnn.py:115-180).  -> ids [B,T_exec] (numpy int32),
        attn_maps [B,H,T_exec,M] (device), logits [B,T_exec,V] or None.
        defer: only enqueue the loop and return a function that fetches the result (the SCST step converts the beam
        rollouts to text on the host while this loop runs); fetch.ids_device / fetch.first_eos_device are then the device
        ids [max_steps,B], whose rows past the executed steps the loop never writes, and the first <EOS> positions [B]
        that say which rows those are (the SCST reward's baseline row takes both)."""
        torch = self.torch
        B = fm.shape[0]
        ctx = self._infer_ctx('greedy', B, 1, max_steps, want_logits, fm, im_embed)

        def launch():
            ctx.desc.flags = L.decoder_flags_from_env()
            L.check(self.lib.comic_decoder_greedy(C.byref(ctx.desc), C.byref(ctx.ptab), ctx.fm.data_ptr(),
                                                  ctx.im.data_ptr(), B, max_steps, ctx.ids.data_ptr(),
                                                  L.ptr(ctx.logits), ctx.hist.data_ptr(), ctx.first_eos.data_ptr(),
                                                  ctx.ws.data_ptr(), ctx.nbytes, L.stream_ptr()), 'decoder_greedy')
        ctx.runner.run(None, launch, use_graph)
        if defer:
            # the ids leave through pinned memory behind an event of their own (as beam_search_ids): the fetch then waits for
            # the rollout, not for whatever the caller has enqueued behind it in the meantime (the SCST step enqueues the
            # update's forward pass before it looks at the greedy captions)
            if ctx.ids_host is None:
                ctx.ids_host = torch.empty((max_steps, B), dtype=torch.int32).pin_memory()
                ctx.eos_host = torch.empty(B, dtype=torch.int32).pin_memory()
                ctx.fetched = torch.cuda.Event()
            ctx.ids_host.copy_(ctx.ids, non_blocking=True)
            ctx.eos_host.copy_(ctx.first_eos, non_blocking=True)
            ctx.fetched.record(torch.cuda.current_stream())

        def fetch():
            if defer:
                ctx.fetched.synchronize()
                fe = ctx.eos_host.numpy()
            else:
                fe = ctx.first_eos.cpu().numpy()
            if fe.min() < 0:                              # comic_persist_check_greedy: a bounded wait of the loop expired
                raise L.ComicHipError('greedy: the persistent decode loop did not complete (a wait on another workgroup timed out)')
            return self._greedy_result(ctx, fe, max_steps, want_logits, ctx.ids_host if defer else None)
        fetch.ids_device, fetch.first_eos_device = ctx.ids, ctx.first_eos
        return fetch if defer else fetch()

    def sample(self, fm, im_embed, max_steps, seed=0, noise=None, want_logits=False):
        """rnn_decoder_search(greedy_search=False) (ops_rnn.py:158-166; ModelBase._rnn_dynamic_decoder(sample=True),
        model_base.py:716-726): SampleEmbeddingHelper draws every next token from Categorical(logits).  The draw is
        argmax(logits + Gumbel noise); `noise` [max_steps,B,V] (device fp32) may be supplied, else it is generated from
        `seed` (torch's generator: the stream is not TensorFlow's Philox, only the distribution is the reference's).
        -> ids [B,T_exec], attn_maps [B,H,T_exec,M], logits [B,T_exec,V] or None, as greedy()."""
        torch, s = self.torch, self.spec
        B = fm.shape[0]
        ctx = self._infer_ctx('greedy', B, 1, max_steps, want_logits, fm, im_embed)
        if noise is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(int(seed))
            u = torch.rand((max_steps, B, s.V), generator=gen, device=self.device, dtype=torch.float32)
            noise = -torch.log(-torch.log(u.clamp_(1e-20, 1.0 - 1e-7)))
        assert tuple(noise.shape) == (max_steps, B, s.V) and noise.dtype == torch.float32 and noise.is_contiguous()
        ctx.desc.flags = L.decoder_flags_from_env()
        L.check(self.lib.comic_decoder_sample(C.byref(ctx.desc), C.byref(ctx.ptab), ctx.fm.data_ptr(), ctx.im.data_ptr(), B,
                                              max_steps, noise.data_ptr(), ctx.ids.data_ptr(), L.ptr(ctx.logits),
                                              ctx.hist.data_ptr(), ctx.first_eos.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes,
                                              L.stream_ptr()), 'decoder_sample')
        return self._greedy_result(ctx, ctx.first_eos.cpu().numpy(), max_steps, want_logits)

    def _greedy_result(self, ctx, first_eos, max_steps, want_logits, ids_host=None):
        """ids [B,T_exec] (numpy), attn_maps [B,H,T_exec,M], logits [B,T_exec,V] or None of a finished greedy / sampled
        loop from its first <EOS> positions (numpy); ids_host: the pinned copy of the ids where they were fetched already."""
        s, B = self.spec, first_eos.shape[0]
        t_exec = int(min(max_steps, first_eos.max() + 1))   # loop ends when every row has emitted EOS
        if ids_host is not None:
            out_ids = np.ascontiguousarray(ids_host[:t_exec].numpy().T)
        else:
            out_ids = ctx.ids[:t_exec].t().contiguous().cpu().numpy()
        hist = ctx.hist[:t_exec].reshape(t_exec, B, s.H, s.M).permute(1, 2, 0, 3).clone()
        return out_ids, hist, (ctx.logits[:t_exec].permute(1, 0, 2).clone() if want_logits else None)

    def _own_ensemble(self):
        """This decoder as a one-member ensemble, the executor of every beam option.  Created at its first use, in
        __dict__: a decoder that never decodes with an option has no such attribute."""
        ens = self.__dict__.get('_self_ensemble')
        if ens is None:
            ens = self._self_ensemble = EnsembleDecoder([self])
        return ens

    def _launch_beam(self, ctx, B, W, max_steps):
        """The comic_decoder_beam call of a 'beam' context (capturable): beam_search_ids' and the plain beam_search's."""
        ctx.desc.flags = L.decoder_flags_from_env()
        L.check(self.lib.comic_decoder_beam(C.byref(ctx.desc), C.byref(ctx.ptab), ctx.fm.data_ptr(), ctx.im.data_ptr(), B, W,
                                            max_steps, ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(),
                                            ctx.scores.data_ptr(), ctx.lengths.data_ptr(), ctx.finished.data_ptr(),
                                            ctx.hist.data_ptr(), ctx.steps.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes,
                                            L.stream_ptr()), 'decoder_beam')

    def beam_search_ids(self, fm, im_embed, beam, max_steps, use_graph=True, slot=0, sampling=None, image_base=0,
                        reward=None, reward_refs=None, reward_baseline_ids=None, prefix=None):
        """Beam search for its predicted ids alone, fetched WITHOUT draining the stream: the loop, gather_tree over all
        max_steps rows (rows past the executed steps come out as end_id) and the copies to pinned memory are enqueued, an
        event marks their end, and the returned function waits for that event only -- work enqueued behind it (the greedy
        rollout of the SCST step) keeps running while the host turns these ids into text.  -> fetch() -> [T,B,W] int32,
        the same values as beam_search()['predicted_ids'].
        sampling: an active BeamSampling draws `beam` samples per image instead (beam_search's sampling= / image_base=).
        reward: a Reward with reward_refs (and reward_baseline_ids for baseline='greedy'): the reward launch follows the
        tree gather on the device ids, all max_steps rows of them; fetch.reward is the dict of its device tensors
        (Decoder.scst_reward; None without) and fetch.ids_device the device ids [max_steps,B,W].
        prefix: a BeamPrefix: every caption starts with its image's row (beam_search's prefix=)."""
        torch, s = self.torch, self.spec
        B, W = fm.shape[0], beam
        opts = BeamOptions(sampling=sampling, image_base=image_base, reward=reward, reward_refs=reward_refs,
                           reward_baseline_ids=reward_baseline_ids, prefix=prefix)
        if sampling is not None or reward is not None or prefix is not None:
            opts.check(s, W, B, max_steps)
        if opts.smp is not None or prefix is not None:
            ctx = self._own_ensemble()._enqueue([fm], [im_embed], W, max_steps, use_graph, opts)
        else:
            ctx = self._infer_ctx('beam', B, W, max_steps, False, fm, im_embed, slot=slot)
            ctx.desc.length_penalty_weight = 0.0
            ctx.runner.run(None, lambda: self._launch_beam(ctx, B, W, max_steps), use_graph)
        if ctx.pred is None:
            ctx.pred = torch.empty((max_steps, B, W), dtype=torch.int32, device=self.device)
            ctx.pred_host = torch.empty((max_steps, B, W), dtype=torch.int32).pin_memory()
            ctx.steps_host = torch.empty(1, dtype=torch.int32).pin_memory()
            ctx.fetched = torch.cuda.Event()
        max_len = ctx.lengths.max(dim=1).values.to(torch.int32).contiguous()
        L.check(self.lib.comic_gather_tree(ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(), max_len.data_ptr(),
                                           ctx.pred.data_ptr(), max_steps, B, W, s.end_id, L.stream_ptr()), 'gather_tree')
        ctx.pred_host.copy_(ctx.pred, non_blocking=True)
        ctx.steps_host.copy_(ctx.steps, non_blocking=True)
        ctx.fetched.record(torch.cuda.current_stream())
        ctx.keep = max_len                                # (alive until the copies have run)

        def fetch():
            ctx.fetched.synchronize()
            return ctx.pred_host[:int(ctx.steps_host[0])].numpy().copy()
        fetch.ids_device, fetch.reward = ctx.pred, None
        if reward is not None:
            fetch.reward = scst_reward(self.lib, torch, ctx.pred, reward_refs, reward,
                                       _baseline_ids(torch, reward_baseline_ids, self.device))
        return fetch

    def beam_search(self, fm, im_embed, beam, max_steps, want_attention=True, use_graph=True, length_penalty_weight=0.0,
                    constraints=None, groups=None, sampling=None, image_base=0, truncation=None, required=None,
                    consensus=None, options=None, reward=None, reward_refs=None, reward_baseline_ids=None, prefix=None):
        """rnn_decoder_beam_search (ops_rnn.py:49-112).  Returns predicted_ids [T,B,W] (after
        gather_tree), scores [T,B,W] (with length_penalty_weight != 0: the penalised scores the beams were ranked by,
        BeamSearchDecoder's `scores` output), the raw step/parent ids and, unless want_attention=False, the
        beam-sorted alignment history [T,B*W,H*M] (numpy; BeamSearchDecoderMultiHead,
        ops_rnn.py:807-845 -- host post-processing that only visualisation needs).
        The options below come as these keywords or as one BeamOptions in `options` (both: ValueError); any active one
        decodes as a one-member ensemble through the one executor entry (comic_decoder_beam_search).
        constraints: a BeamConstraints; None / inactive ones change nothing.
        groups: a BeamGroups (diverse beam search); an active one (groups > 1) decodes alone or with constraints: slot g * (beam / groups) of predicted_ids and scores is
        group g's best caption, and the result carries `log_probs` [B,W] (BeamGroups.final_log_probs).  None / inactive:
        today's path.  The result's `groups` holds the number of groups (1 without).
        sampling: a BeamSampling; an active one draws `beam` samples per image, alone or with
        constraints (not with more than one group or a length penalty: ValueError): slot w of predicted_ids is sample
        w, `scores` the chains' running log p(caption | image) and `log_probs` [B,beam] the final ones; image_base is the
        index in the run of the batch's first image (the noise of an image does not depend on its batch).  None /
        inactive: today's path.
        truncation: a BeamTruncation; an active one (with active sampling: ValueError otherwise) restricts every draw to the
        top_k likeliest tokens and / or the top_p nucleus.  `scores` / `log_probs` stay
        the model's own unperturbed, untempered, UNTRUNCATED log p(caption | image) -- Decoder.score reproduces them -- not
        the log-probability under the truncated distribution.  None / inactive: today's path, call for call.
        required: a BeamRequired (one row of words per image); decodes by banks, alone or with
        constraints and a length penalty (not with groups or sampling: ValueError).  Slot c * (beam / banks) of
        predicted_ids and scores is bank c's best; the result gains `banks`, `best_slot` [B] (the caption's slot: the
        highest bank that holds a hypothesis) and `met` [B] (the required words that bank stands for, padding included),
        and `log_probs` [B,W], the final unpenalised log-probabilities.  None: today's path.
        consensus: a Consensus; one comic_caption_consensus launch on the device ids right after the tree gather, outside
        the captured graph, with every decode above: the result gains `consensus` [B,W] float64, every candidate's mean
        CIDEr-D similarity to its siblings, and `consensus_best` [B] int32, the slot of the largest.  The posterior
        weights read `log_probs` (without groups, sampling or required words: the last `scores`); with required= they
        are forced, so that a dead slot (-inf) neither votes nor is chosen.  None: today's path, launch for launch.
        reward: a Reward, with reward_refs (the RewardRefs of the batch) and, for baseline='greedy', reward_baseline_ids
        [T0,B]: one comic_scst_reward launch on the device ids right after the tree gather, outside the captured graph,
        with every decode above: the result gains `reward` [B,W'] float64, `advantage` [W,B] float32 and `reward_device`,
        the operator's device tensors (Decoder.scst_reward).  None: today's path, launch for launch.
        prefix: a BeamPrefix (one row of tokens per image, -1 padded); every caption of image b starts with row b, with
        every decode above (comic_decoder_beam_search_prefixed).  `scores` / `log_probs` stay the model's
        log p(prefix + continuation | image) -- Decoder.score of the whole caption reproduces them -- and lengths count the
        forced tokens.  Inside the prefix the slots that do not carry it hold -inf (plain beam and groups: all but the
        first of each group).  The result gains `log_probs` [B,W] where it has none (the plain beam's final unpenalised
        totals) and `prefix_log_prob` [B,W], log p(prefix | image) of every slot's caption
        (BeamPrefix.prefix_log_probs).  None: today's path, context for context."""
        opts = BeamOptions.of(options, length_penalty_weight=length_penalty_weight, constraints=constraints, groups=groups,
                              sampling=sampling, truncation=truncation, required=required, consensus=consensus,
                              image_base=image_base, reward=reward, reward_refs=reward_refs,
                              reward_baseline_ids=reward_baseline_ids, prefix=prefix)
        B, W = fm.shape[0], beam
        opts.check(self.spec, W, B, max_steps)
        if opts.active:
            return self._own_ensemble()._decode([fm], [im_embed], W, max_steps, want_attention, use_graph, opts)
        # (a non-zero length penalty is another captured graph: the weight is baked into the step kernel's arguments)
        lpw = float(opts.length_penalty_weight)
        ctx = self._infer_ctx('beam' if not lpw else 'beam_lp%r' % lpw, B, W, max_steps, False, fm, im_embed)
        ctx.desc.length_penalty_weight = lpw
        ctx.runner.run(None, lambda: self._launch_beam(ctx, B, W, max_steps), use_graph)
        return _beam_result(self, ctx, B, W, opts, want_attention)

    def consensus(self, ids, cons, log_probs=None):
        """The raw consensus operator (comic_caption_consensus) on ids [T,B,W], a device tensor or a numpy array of
        candidates as the tree gather leaves them, under the Consensus `cons`; log_probs [B,W] (float32) is what
        weights='posterior' reads.  -> (utility [B,W] float64, best [B] int32), numpy."""
        torch = self.torch
        ids = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids, np.int32))
        if ids.dim() != 3:
            raise ValueError('consensus: ids must be [T, B, W], got shape %r' % (tuple(ids.shape),))
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        if log_probs is not None:
            lp = log_probs if torch.is_tensor(log_probs) else torch.from_numpy(np.ascontiguousarray(log_probs, np.float32))
            log_probs = lp.to(device=self.device, dtype=torch.float32).contiguous()
        util, best = caption_consensus(self.lib, torch, ids, self.spec.end_id, cons, log_probs)
        return util.cpu().numpy(), best.cpu().numpy()

    def scst_reward(self, ids, refs, reward, baseline_ids=None, baseline_first_eos=None):
        """The raw reward operator (comic_scst_reward) on ids [T,B,W] and baseline_ids [T0,B] or None, device tensors or
        numpy arrays of rollouts as the tree gather / the greedy decode leave them, against the RewardRefs `refs` under the
        Reward `reward`.  -> dict of DEVICE tensors: cider [B,W'], bleu [B,W',4], reward [B,W'], baseline [B,W] (float64)
        and advantage [W,B] (float32; .reshape(-1) is what train_step(rewards=) takes).  Nothing is synchronised."""
        torch = self.torch

        def dev(a, nd, what):
            a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.int32))
            if a.dim() != nd:
                raise ValueError('scst_reward: %s must have %d dimensions, got shape %r' % (what, nd, tuple(a.shape)))
            return a.to(device=self.device, dtype=torch.int32).contiguous()
        ids = dev(ids, 3, 'ids')
        if baseline_ids is not None:
            baseline_ids = dev(baseline_ids, 2, 'baseline_ids')
        if baseline_first_eos is not None:
            baseline_first_eos = dev(baseline_first_eos, 1, 'baseline_first_eos')
        return scst_reward(self.lib, torch, ids, refs, reward, baseline_ids, baseline_first_eos)


def _gather_tree_host(step_ids, parent_ids, max_len, end_token):
    T, B, W = parent_ids.shape
    beams = np.full((T, B, W), end_token, np.int32)
    for b in range(B):
        Lb = min(T, int(max_len[b]))
        if Lb <= 0:
            continue
        for w in range(W):
            beams[Lb - 1, b, w] = step_ids[Lb - 1, b, w]
            parent = parent_ids[Lb - 1, b, w]
            for level in range(Lb - 2, -1, -1):
                beams[level, b, w] = step_ids[level, b, parent]
                parent = parent_ids[level, b, parent]
            fin = False
            for t in range(Lb):
                if fin:
                    beams[t, b, w] = end_token
                elif beams[t, b, w] == end_token:
                    fin = True
    return beams


def gather_tree_from_array(t, parent_ids, sequence_length, _unused_end=None):
    """Beam-sort a per-step state array [T, B*W, S] (BeamSearchDecoderMultiHead.
    _maybe_sort_array_beams, ops_rnn.py:807-845 -> [TF-1.9] gather_tree_from_array).
    Host post-processing of the alignment history (small, index-only)."""
    T, B, W = parent_ids.shape
    beam_ids = np.tile(np.arange(W, dtype=np.int32)[None, None, :], (T, B, 1))
    mask = (np.arange(T)[None, None, :] < np.asarray(sequence_length)[:, :, None]).transpose(2, 0, 1)
    masked = np.where(mask, beam_ids, W + 1).astype(np.int32)
    max_len = np.asarray(sequence_length).max(axis=1)
    sorted_ids = _gather_tree_host(masked, parent_ids, max_len, W + 1)
    sorted_ids = np.where(mask, sorted_ids, beam_ids)
    src = np.asarray(t).reshape(T, B, W, -1)
    return src[np.arange(T)[:, None, None], np.arange(B)[None, :, None], sorted_ids].reshape(np.asarray(t).shape)


def check_ensemble(specs, weights=None):
    """Validation of an ensemble on the host (no GPU call): 1 to 8 members that agree in vocabulary size, token type and
    start / end ids; weights (default uniform) one per member, >= 0, summing to 1 within 1e-6.  -> the weights as a list."""
    n = len(specs)
    if not 1 <= n <= 8:
        raise ValueError('an ensemble has 1 to 8 members, got %d' % n)
    for k, s in enumerate(specs[1:], 1):
        for f in ('V', 'token_type', 'start_id', 'end_id'):
            if getattr(s, f) != getattr(specs[0], f):
                raise ValueError('ensemble member %d differs from member 0 in %s: %r against %r'
                                 % (k, f, getattr(s, f), getattr(specs[0], f)))
    if weights is None:
        return [1.0 / n] * n
    w = [float(x) for x in weights]
    if len(w) != n:
        raise ValueError('%d ensemble weights for %d members' % (len(w), n))
    if any(not (x >= 0.0) or math.isinf(x) for x in w):
        raise ValueError('ensemble weights must be finite and >= 0: %r' % (w,))
    if abs(sum(w) - 1.0) > 1e-6:
        raise ValueError('ensemble weights must sum to 1 (got %r)' % (sum(w),))
    return w


class EnsembleDecoder:
    """Several decoders, one beam: beam search whose step distribution is the weighted mean of the members' word
    distributions (comic_decoder_beam_ensemble; extends rnn_decoder_beam_search, ops_rnn.py:49-112).  Members may differ
    in geometry, cell and attention; they share the vocabulary."""

    def __init__(self, decoders, weights=None):
        decoders = list(decoders)
        self.weights = check_ensemble([d.spec for d in decoders], weights)      # raises before anything touches the GPU
        self.decoders = decoders
        self.spec = decoders[0].spec
        self.torch, self.lib, self.device = decoders[0].torch, decoders[0].lib, decoders[0].device
        self._ctxs = {}

    def teacher_targets(self, fm, im_embed, captions, top_k=16, temperature=1.0, weights=None):
        """The ensemble as a teacher: ids, probs [T,B,top_k] of the members' weighted mean tempered softmax on the captions'
        teacher-forced rows (teacher_table); every member reads the same fm / im_embed.  weights: the ensemble's, or these."""
        w = self.weights if weights is None else check_ensemble([d.spec for d in self.decoders], weights)
        return teacher_table(self.decoders, w, fm, im_embed, captions, top_k, temperature)

    def _ctx(self, B, W, max_steps, feats, opts):
        """Persistent buffers (+ a hipGraph of the whole loop, captured on the second call with the shape), as
        Decoder._infer_ctx, keyed by the shape and opts.ctx_key(): what the captured launches bake in.  What they do not --
        the seed words and the required table -- lives in ctx.seed and ctx.req, which _decode writes in front of every
        launch."""
        torch, n = self.torch, len(self.decoders)
        key = (B, W, max_steps, opts.context_key())
        ctx = self._ctxs.get(key)
        if ctx is None:
            ctx = _DecodeContext(torch, key)
            R = B * W
            f32 = dict(dtype=torch.float32, device=self.device)
            specs = [d.spec for d in self.decoders]
            ctx.fm = [torch.empty((B, s.M, s.C), **f32) for s in specs]
            ctx.im = [torch.empty((B, s.Cg), **f32) for s in specs]
            ctx.hist = torch.empty((max_steps, R, specs[0].H * specs[0].M), **f32)      # member 0's alignments
            _beam_outputs(ctx, torch, self.device, B, W, max_steps)
            ctx.descs = (L.DecoderDesc * n)(*[s.desc(False) for s in specs])
            ctx.descs[0].length_penalty_weight = float(opts.length_penalty_weight)
            ctx.ptabs = (L.DecoderParams * n)(*[d.params.table() for d in self.decoders])
            ctx.fm_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ctx.fm])
            ctx.im_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ctx.im])
            ctx.hist_ptrs = (C.c_void_p * n)(*([ctx.hist.data_ptr()] + [None] * (n - 1)))
            ctx.wts = (C.c_float * n)(*self.weights)
            if opts.smp is not None:
                ctx.seed = torch.zeros(2, dtype=torch.int64, device=self.device)       # uint64[2]: {seed, image_base}
            if opts.required is not None:
                ctx.req = torch.full((B, opts.required.n_words, opts.required.stride), -1, dtype=torch.int32,
                                     device=self.device)
            ctx.options = opts.c_record(ctx)
            if opts.prefix is None:
                ctx.nbytes = int(self.lib.comic_decoder_beam_search_workspace(ctx.descs, n, R, max_steps,
                                                                              C.byref(ctx.options)))
            else:
                ctx.prefix = opts.prefix.c_struct()
                ctx.pfx = torch.full((B, opts.prefix.max_tokens), -1, dtype=torch.int32, device=self.device)
                ctx.nbytes = int(self.lib.comic_decoder_beam_search_prefixed_workspace(
                    ctx.descs, n, R, max_steps, C.byref(ctx.options), C.byref(ctx.prefix)))
            assert ctx.nbytes > 0, 'the ensemble workspace query failed'
            ctx.ws = torch.empty(ctx.nbytes, dtype=torch.uint8, device=self.device)
            self._ctxs[key] = ctx
        for k, (fm, im) in enumerate(feats):
            ctx.fm[k].copy_(fm.reshape(ctx.fm[k].shape))
            ctx.im[k].copy_(im.reshape(ctx.im[k].shape))
        return ctx

    def beam_search(self, fms, im_embeds, beam, max_steps, want_attention=False, use_graph=True, length_penalty_weight=0.0,
                    constraints=None, groups=None, sampling=None, image_base=0, truncation=None, required=None,
                    consensus=None, options=None, reward=None, reward_refs=None, reward_baseline_ids=None, prefix=None):
        """fms / im_embeds: one device tensor (every member reads the same features) or a sequence with one per member.
        Returns the dict of Decoder.beam_search; `attn_hist` (want_attention) is member 0's.  The options -- these keywords
        or one BeamOptions in `options` -- are Decoder.beam_search's and mean what they mean there; every decode runs
        through comic_decoder_beam_search, and None / inactive options are the plain ensemble decode, launch for launch."""
        opts = BeamOptions.of(options, length_penalty_weight=length_penalty_weight, constraints=constraints, groups=groups,
                              sampling=sampling, truncation=truncation, required=required, consensus=consensus,
                              image_base=image_base, reward=reward, reward_refs=reward_refs,
                              reward_baseline_ids=reward_baseline_ids, prefix=prefix)
        torch, n = self.torch, len(self.decoders)
        if torch.is_tensor(fms):
            fms = [fms] * n
        if torch.is_tensor(im_embeds):
            im_embeds = [im_embeds] * n
        opts.check(self.spec, beam, int(fms[0].shape[0]), max_steps)
        return self._decode(fms, im_embeds, beam, max_steps, want_attention, use_graph, opts)

    def _decode(self, fms, im_embeds, beam, max_steps, want_attention, use_graph, opts):
        """The decode of checked options: one feature tensor per member."""
        ctx = self._enqueue(fms, im_embeds, beam, max_steps, use_graph, opts)
        return _beam_result(self, ctx, int(fms[0].shape[0]), int(beam), opts, want_attention)

    def _enqueue(self, fms, im_embeds, beam, max_steps, use_graph, opts):
        """The launches of a decode of checked options, without a fetch -> its context."""
        torch, n = self.torch, len(self.decoders)
        assert len(fms) == n and len(im_embeds) == n
        B, W, max_steps = int(fms[0].shape[0]), int(beam), int(max_steps)
        ctx = self._ctx(B, W, max_steps, list(zip(fms, im_embeds)), opts)
        if opts.required is not None:       # on the stream, in front of the launch or the replay that reads it
            ctx.req.copy_(torch.from_numpy(opts.required.ids))
        if opts.smp is not None:            # on the stream, in front of the launch or the replay that reads them
            ctx.seed.copy_(torch.from_numpy(opts.smp.seed_words(opts.image_base)))
        if opts.prefix is not None:         # likewise: the graph bakes in the table's width, not its content
            ctx.pfx.copy_(torch.from_numpy(opts.prefix.ids))

        def launch():
            flags = L.decoder_flags_from_env()
            for k in range(n):
                ctx.descs[k].flags = flags
            outs = (ctx.step_ids.data_ptr(), ctx.parent_ids.data_ptr(), ctx.scores.data_ptr(), ctx.lengths.data_ptr(),
                    ctx.finished.data_ptr(), ctx.hist_ptrs, ctx.steps.data_ptr(), ctx.ws.data_ptr(), ctx.nbytes,
                    L.stream_ptr())
            if ctx.prefix is None:
                L.check(self.lib.comic_decoder_beam_search(
                    ctx.descs, ctx.ptabs, ctx.fm_ptrs, ctx.im_ptrs, ctx.wts, n, B, W, max_steps, C.byref(ctx.options),
                    *outs), 'decoder_beam_search')
            else:
                L.check(self.lib.comic_decoder_beam_search_prefixed(
                    ctx.descs, ctx.ptabs, ctx.fm_ptrs, ctx.im_ptrs, ctx.wts, n, B, W, max_steps, C.byref(ctx.options),
                    C.byref(ctx.prefix), ctx.pfx.data_ptr(), *outs), 'decoder_beam_search_prefixed')
        ctx.runner.run(None, launch, use_graph)
        return ctx
