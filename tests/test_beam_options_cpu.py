"""The one options record of beam search on the host (no GPU compute): comic_beam_options and its two entries in the header
and the library, the workspace of every legal combination against the named per-option queries and against
tests/golden/beam_workspace_sizes.json (the named queries' results, recorded from the build before the record existed),
the executor's refusals, and decoder.BeamOptions: its checks, its context key, and the configuration functions."""
import ctypes as C
import dataclasses
import itertools
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import comic_amd._lib as L
from comic_amd import decoder as cdec
from comic_amd.decoder import (BeamConstraints, BeamGroups, BeamOptions, BeamRequired, BeamSampling, BeamTruncation,
                               Consensus)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'beam_workspace_sizes.json')))
NEW_SYMBOLS = ('comic_decoder_beam_search_workspace', 'comic_decoder_beam_search')
# the ten legal combinations: the options present, and the named query of that combination with its `constrained` flag
COMBOS = {'none': ((), 'ensemble', None), 'cons': (('constraints',), 'constrained', None),
          'grp': (('groups',), 'diverse', 0), 'cons+grp': (('constraints', 'groups'), 'diverse', 1),
          'smp': (('sampling',), 'sampled', 0), 'cons+smp': (('constraints', 'sampling'), 'sampled', 1),
          'smp+trc': (('sampling', 'truncation'), 'truncated', 0),
          'cons+smp+trc': (('constraints', 'sampling', 'truncation'), 'truncated', 1),
          'rqd': (('required',), 'required', 0), 'cons+rqd': (('constraints', 'required'), 'required', 1)}
STRUCTS = dict(constraints=L.BeamConstraints, groups=L.BeamGroups, sampling=L.BeamSampling, truncation=L.BeamTruncation,
               required=L.BeamRequired)


def _record(present, keep, **fields):
    """A comic_beam_options whose `present` options point at structs (parked in `keep`) with the given fields."""
    rec = L.BeamOptions()
    for name in present:
        s = STRUCTS[name](**fields.get(name, {}))
        keep.append(s)
        setattr(rec, name, C.addressof(s))
    return rec


def _descs(n, V):
    return (L.DecoderDesc * n)(*[cdec.DecoderSpec(V=V, **GOLDEN['spec']).desc(False) for _ in range(n)])


def test_new_entries_are_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'comic_hip.h')).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r'\b%s\(' % name, header)
        assert m, name
        assert 'ops_rnn.py:49-112' in header[max(0, m.start() - 2500):m.start()], name
    assert '#define COMIC_ABI_VERSION 1' in header               # additive change
    fields = re.search(r'typedef struct comic_beam_options \{(.*?)\} comic_beam_options;', re.sub(r'/\*.*?\*/', '', header, flags=re.S),
                       re.S).group(1)
    assert fields.split() == ('const comic_beam_constraints* constraints; const comic_beam_groups* groups; '
                              'const comic_beam_sampling* sampling; const comic_beam_truncation* truncation; '
                              'const comic_beam_required* required; const int32_t* req;').split()
    assert C.sizeof(L.BeamOptions) == 6 * 8


def test_grid_of_the_recorded_sizes():
    grid = {(c['n'], c['rows'], c['max_steps'], c['V']) for c in GOLDEN['cases']}
    assert grid == set(itertools.product((1, 2), (8, 150), (6, 30), (258, 25599)))
    assert all(set(c['bytes']) == set(COMBOS) for c in GOLDEN['cases'])


@pytest.mark.parametrize('case', GOLDEN['cases'], ids=lambda c: 'n%d-rows%d-steps%d-V%d' % (c['n'], c['rows'], c['max_steps'], c['V']))
def test_workspace_of_every_legal_combination_is_the_named_query(case):
    lib = L.load()
    n, rows, steps = case['n'], case['rows'], case['max_steps']
    descs = _descs(n, case['V'])
    for combo, (present, named, flag) in COMBOS.items():
        keep = []
        rec = _record(present, keep)
        got = lib.comic_decoder_beam_search_workspace(descs, n, rows, steps, C.byref(rec))
        query = getattr(lib, 'comic_decoder_beam_%s_workspace' % named)
        assert got == query(descs, n, rows, steps, *(() if flag is None else (flag,))) == case['bytes'][combo] > 0, combo
    assert lib.comic_decoder_beam_search_workspace(descs, n, rows, steps, None) == case['bytes']['none']     # a NULL record


def test_workspace_is_minus_one_where_the_named_query_is():
    lib = L.load()
    descs = _descs(2, 258)
    for combo, (present, named, flag) in COMBOS.items():
        keep = []
        rec = _record(present, keep)
        query = getattr(lib, 'comic_decoder_beam_%s_workspace' % named)
        tail = () if flag is None else (flag,)
        for d, n, rows, steps in ((None, 2, 8, 6), (descs, 0, 8, 6), (descs, 9, 8, 6), (descs, 2, 0, 6), (descs, 2, 8, 0),
                                  (descs, 2, 8, -3)):
            want = query(d, n, rows, steps, *tail)
            assert lib.comic_decoder_beam_search_workspace(d, n, rows, steps, C.byref(rec)) == want, (combo, n, rows, steps)
            if d is None or n in (0, 9) or rows == 0 or (steps <= 0 and ('constraints' in present or 'required' in present)):
                assert want == -1, (combo, n, rows, steps)
    bad = _descs(1, 258)
    bad[0].V = 0
    assert lib.comic_decoder_beam_search_workspace(bad, 1, 8, 6, None) == -1


@pytest.mark.parametrize('present,fields,req,what', [
    (('groups', 'required'), dict(groups=dict(groups=2, diversity=0.5)), 1, 'groups = 2 does not combine with required words'),
    (('sampling', 'required'), {}, 1, 'sampling does not combine with required words'),
    (('groups', 'sampling'), dict(groups=dict(groups=2, diversity=0.5)), 0, 'sampling does not combine with groups = 2'),
    (('truncation',), {}, 0, 'null sampling'),
    (('constraints', 'truncation'), {}, 0, 'null sampling'),
    (('required',), {}, 0, 'null req table'),
])
def test_the_entry_refuses_illegal_records_before_it_reads_anything_else(present, fields, req, what):
    """With null descs (and every other pointer null): a legal record gets as far as the null-pointer check, an illegal one
    is refused with its own message first."""
    lib = L.load()
    keep = []
    rec = _record(present, keep, **fields)
    rec.req = 0x1000 if req else None                             # (never read: the refusal comes first)

    def call(r):
        return lib.comic_decoder_beam_search(None, None, None, None, None, 1, 2, 4, 6, r, None, None, None, None, None, None,
                                             None, None, 0, None)
    assert call(C.byref(rec)) != 0
    assert what in lib.comic_last_error().decode(), lib.comic_last_error()
    one_group = _record(('groups', 'required'), keep, groups=dict(groups=1))      # one group is no groups: legal beside
    one_group.req = 0x1000                                                        # required words and beside sampling
    one_group_sampled = _record(('groups', 'sampling', 'truncation'), keep, groups=dict(groups=1))
    for legal in (None, C.byref(one_group), C.byref(one_group_sampled)):
        assert call(legal) != 0 and 'beam_ensemble: null pointer' in lib.comic_last_error().decode()


# ---- decoder.BeamOptions -----------------------------------------------------------------------------------------------------
SPEC = SimpleNamespace(V=258, end_id=257)
RQD = BeamRequired(np.array([[[7]], [[9]]], np.int32))


@pytest.mark.parametrize('kw,what', [
    (dict(sampling=BeamSampling(0.7, 3), groups=BeamGroups(2, 0.5)), 'beam groups'),
    (dict(sampling=BeamSampling(0.7, 3), length_penalty_weight=0.7), 'length penalty'),
    (dict(truncation=BeamTruncation(5)), 'needs an active BeamSampling'),
    (dict(truncation=BeamTruncation(5), sampling=BeamSampling(0.7, 3, enabled=False)), 'needs an active BeamSampling'),
    (dict(required=RQD, groups=BeamGroups(2, 0.5)), 'do not combine with beam groups'),
    (dict(required=RQD, sampling=BeamSampling(0.7, 3)), 'do not combine with sampling'),
])
def test_check_refuses_every_illegal_pair(kw, what):
    with pytest.raises(ValueError, match=what):
        BeamOptions(**kw).check(SPEC, 4, 2, 10)


def test_check_passes_the_legal_combinations_and_keeps_decoders_order():
    cons, smp = BeamConstraints(min_length=2, no_repeat_ngram=2), BeamSampling(0.7, 3)
    for kw in (dict(), dict(constraints=cons), dict(groups=BeamGroups(2, 0.5)), dict(constraints=cons, groups=BeamGroups(2, 0.5)),
               dict(sampling=smp), dict(constraints=cons, sampling=smp), dict(sampling=smp, truncation=BeamTruncation(5, 0.9)),
               dict(required=RQD), dict(required=RQD, constraints=cons, length_penalty_weight=0.7, groups=BeamGroups(1, 0.5)),
               dict(sampling=smp, consensus=Consensus())):
        BeamOptions(**kw).check(SPEC, 4, 2, 10)
    # consensus, truncation, required, groups, sampling, then the active constraints: the first broken rule speaks
    broken = dict(consensus=Consensus(sigma=0.0), truncation=BeamTruncation(-1), required=BeamRequired(np.zeros((3, 1, 1), np.int32)),
                  groups=BeamGroups(3, 0.5), sampling=BeamSampling(0.0, 1), constraints=BeamConstraints(min_length=99))
    order = ('consensus', 'truncation', 'required', 'groups', 'sampling', 'constraints')
    for k, what in zip(range(len(order)), ('sigma', 'top_k', 'the table holds 3 images', 'does not divide', 'temperature', 'min_length')):
        with pytest.raises(ValueError, match=what):
            BeamOptions(**{name: broken[name] for name in order[k:]}).check(SPEC, 4, 2, 10)


def test_of_takes_the_record_or_the_keywords_not_both():
    smp = BeamSampling(0.7, 3)
    defaults = dict(length_penalty_weight=0.0, groups=None, constraints=None, sampling=None, truncation=None, required=None,
                    consensus=None, image_base=0)
    assert BeamOptions.of(None, **dict(defaults, sampling=smp, image_base=9)) == BeamOptions(sampling=smp, image_base=9)
    given = BeamOptions(sampling=smp)
    assert BeamOptions.of(given, **defaults) is given
    for k, v in (('sampling', smp), ('length_penalty_weight', 0.7), ('image_base', 4), ('groups', BeamGroups())):
        with pytest.raises(ValueError, match='not both'):
            BeamOptions.of(given, **dict(defaults, **{k: v}))
    with pytest.raises(Exception):
        given.sampling = None                                     # immutable


def test_active_decides_between_the_two_executors():
    assert not BeamOptions().active and not BeamOptions(length_penalty_weight=0.7, consensus=Consensus()).active
    assert not BeamOptions(constraints=BeamConstraints(), groups=BeamGroups(1, 0.5), sampling=BeamSampling(enabled=False),
                           truncation=BeamTruncation()).active
    for kw in (dict(constraints=BeamConstraints(min_length=1)), dict(groups=BeamGroups(2, 0.0)), dict(sampling=BeamSampling()),
               dict(required=RQD)):
        assert BeamOptions(**kw).active, kw


def test_ctx_key_holds_what_a_graph_bakes_in_and_nothing_else():
    plain = BeamOptions().ctx_key()
    assert plain == (0.0, None, None, None, None, None)
    for kw in (dict(constraints=BeamConstraints()), dict(groups=BeamGroups()), dict(groups=BeamGroups(1, 0.5)),
               dict(sampling=BeamSampling(enabled=False)), dict(sampling=BeamSampling(0.3, 5, enabled=False)),
               dict(truncation=BeamTruncation()), dict(consensus=Consensus()), dict(image_base=7),
               dict(constraints=BeamConstraints(), groups=BeamGroups(1, 0.5), sampling=BeamSampling(enabled=False),
                    truncation=BeamTruncation(), image_base=3)):
        assert BeamOptions(**kw).ctx_key() == plain, kw
    keys = [BeamOptions(**kw).ctx_key() for kw in (
        dict(), dict(length_penalty_weight=0.7), dict(constraints=BeamConstraints(min_length=2)),
        dict(constraints=BeamConstraints(min_length=3)), dict(groups=BeamGroups(2, 0.5)), dict(groups=BeamGroups(2, 0.25)),
        dict(sampling=BeamSampling(0.7)), dict(sampling=BeamSampling(0.8)), dict(sampling=BeamSampling(0.7), truncation=BeamTruncation(5)),
        dict(sampling=BeamSampling(0.7), truncation=BeamTruncation(6)), dict(sampling=BeamSampling(0.7), truncation=BeamTruncation(5, 0.9)),
        dict(required=RQD), dict(required=BeamRequired(np.zeros((2, 2, 1), np.int32))),
        dict(required=RQD, constraints=BeamConstraints(min_length=2)))]
    assert len(set(keys)) == len(keys) and all(len(k) == len(plain) for k in keys)
    # written in front of every launch, so not in the key: the seed, image_base, the required table
    assert BeamOptions(sampling=BeamSampling(0.7, 3)).ctx_key() == BeamOptions(sampling=BeamSampling(0.7, 4), image_base=50).ctx_key()
    assert BeamOptions(required=RQD).ctx_key() == BeamOptions(required=BeamRequired(np.array([[[11]], [[-1]]], np.int32))).ctx_key()
    # the floats as the fp32 values the kernels see
    assert BeamOptions(sampling=BeamSampling(0.7)).ctx_key() == BeamOptions(sampling=BeamSampling(0.7 + 1e-12)).ctx_key()
    assert BeamOptions(sampling=BeamSampling(0.7)).ctx_key() != BeamOptions(sampling=BeamSampling(0.7 + 1e-6)).ctx_key()
    t = lambda p: BeamOptions(sampling=BeamSampling(0.7), truncation=BeamTruncation(5, p)).ctx_key()     # noqa: E731
    assert t(0.9) == t(0.9 + 1e-12) and t(0.9) != t(float(np.nextafter(np.float32(0.9), np.float32(1.0))))


def test_c_record_points_at_the_active_options_kept_on_the_context():
    ctx = SimpleNamespace(seed=SimpleNamespace(data_ptr=lambda: 0x2000), req=SimpleNamespace(data_ptr=lambda: 0x3000))
    rec = BeamOptions(constraints=BeamConstraints(min_length=2), groups=BeamGroups(1, 0.5), sampling=BeamSampling(0.5, 3),
                      truncation=BeamTruncation(5, 0.9)).c_record(ctx)
    assert (rec.constraints, rec.sampling, rec.truncation) == tuple(C.addressof(x) for x in (ctx.cons, ctx.smp, ctx.trc))
    assert rec.groups is None and ctx.grp is None and rec.required is None and ctx.rqd is None and rec.req is None
    assert (ctx.cons.min_length, ctx.smp.temperature, ctx.smp.seed_dev, ctx.trc.top_k) == (2, 0.5, 0x2000, 5)
    rec = BeamOptions(required=RQD).c_record(ctx)
    assert rec.required == C.addressof(ctx.rqd) and rec.req == 0x3000 and (ctx.rqd.n_words, ctx.rqd.stride) == (1, 1)
    assert ctx.smp is None and rec.sampling is None


# ---- the configuration -------------------------------------------------------------------------------------------------------
def _config(**kw):
    return SimpleNamespace(**dict(dict(infer_beam_size=4, infer_max_length=20, token_type='word', radix_base=256,
                                       wtoi={'a': 0, 'b': 1, 'c': 2, '<GO>': 3, '<EOS>': 4}), **kw))


CONFIGS = [dict(), dict(infer_min_length=3, infer_no_repeat_ngram=2), dict(infer_beam_groups=2, infer_diversity=0.5),
           dict(infer_sample=True, infer_temperature=0.7, infer_sample_seed=3),
           dict(infer_sample=True, infer_top_k=40, infer_top_p=0.9, infer_consensus=True),
           dict(infer_min_length=3, infer_suppress_words='a,b', infer_sample=True, infer_top_p=0.5),
           dict(infer_temperature=0.7), dict(infer_length_penalty_weight=0.7, infer_beam_groups=4)]


@pytest.mark.parametrize('kw', CONFIGS)
def test_decode_dir_suffix_is_the_six_suffixes_in_order(kw):
    c = _config(**kw)
    assert cdec.decode_dir_suffix(c) == (cdec.constraints_dir_suffix(c) + cdec.groups_dir_suffix(c) + cdec.sampling_dir_suffix(c)
                                         + cdec.truncation_dir_suffix(c) + cdec.consensus_dir_suffix(c)
                                         + cdec.required_dir_suffix(c))


def test_decode_dir_suffix_with_required_words(tmp_path):
    path = tmp_path / 'words.json'
    path.write_text(json.dumps({'img_1.jpg': ['a']}))
    c = _config(infer_require_file=str(path), infer_min_length=2)
    assert cdec.decode_dir_suffix(c) == '_min2_ngram0_sup0_req1_words'
    opts = cdec.options_from_config(c)
    assert opts.required is None and opts.constraints == BeamConstraints(min_length=2)       # the rows come per batch
    with pytest.raises(ValueError, match='infer_beam_size 3 is no multiple of 2'):
        cdec.options_from_config(_config(infer_require_file=str(path), infer_beam_size=3), load=False)


@pytest.mark.parametrize('kw', CONFIGS)
def test_options_from_config_is_the_per_option_functions(kw):
    c = _config(**kw)
    opts = cdec.options_from_config(c)
    assert opts == BeamOptions(kw.get('infer_length_penalty_weight', 0.0), cdec.constraints_from_config(c),
                               cdec.groups_from_config(c), cdec.sampling_from_config(c), cdec.truncation_from_config(c), None,
                               cdec.consensus_from_config(c))
    assert opts.image_base == 0 and opts.required is None
    early = cdec.options_from_config(c, load=False)              # what the command line checks before it loads anything
    assert early.constraints is None and early == dataclasses.replace(opts, constraints=None)


@pytest.mark.parametrize('kw,what', [
    (dict(infer_beam_groups=3), 'does not divide'), (dict(infer_sample=True, infer_beam_groups=2), 'beam groups'),
    (dict(infer_sample=True, infer_length_penalty_weight=0.7), 'length penalty'), (dict(infer_top_k=5), 'set infer_sample'),
    (dict(infer_consensus=True), 'set infer_sample'), (dict(infer_consensus_df='x.p'), 'set infer_consensus'),
])
def test_options_from_config_raises_what_the_command_line_raised(kw, what):
    for load in (False, True):
        with pytest.raises(ValueError, match=what):
            cdec.options_from_config(_config(**kw), load=load)
