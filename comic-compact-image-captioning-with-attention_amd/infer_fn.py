"""Inference driver with the reference's entry points (src/infer_fn.py): `id_to_caption`,
`run_inference`, `evaluate_model` and the same output files (`captions___N.json`,
`outputs___N.pkl`, `infer_speed.txt`; infer_fn.py:166-184).  The Java COCO scorers
(METEOR / SPICE / PTB tokenizer) are outside the hot path: `evaluate_model`
runs inference and hands the JSON to an evaluator callable -- `comic_amd.coco_eval.evaluate_captions`
(native BLEU-1..4 / ROUGE-L / CIDEr, pinned against the reference's Python scorers) when infer.py finds the
annotation file."""
from __future__ import annotations

import json
import os
import pickle
import re
import time

import numpy as np

from . import decoder as cdec, inputs, model as mdl
from .ops import id_to_caption, base_n_to_dec as _baseN_arr_to_dec  # noqa: F401  (re-exported)

pjoin = os.path.join
P_COCO = re.compile(r'(?<=_)\d+')
P_CKPT = re.compile(r'\d+')


def run_inference(config, curr_ckpt_path, device='cuda:0'):
    """Main inference function. Builds and executes the model."""
    ckpt_dir, ckpt_file = os.path.split(curr_ckpt_path)
    ckpt_num = P_CKPT.findall(ckpt_file)[0]
    mdl.reset_default_graph()
    inputs_man = inputs.InputManager(config, is_inference=True)
    try:
        return _inference_loop(inputs_man, curr_ckpt_path, ckpt_dir, ckpt_file, ckpt_num, device)
    finally:
        inputs_man.close()


def ensemble_name(ckpt_nums):
    """Tag of an ensemble's output files: captions___ens_<n1>+<n2>+....json"""
    return 'ens_' + '+'.join(str(n) for n in ckpt_nums)


def run_inference_ensemble(config, ckpt_paths, weights=None, device='cuda:0'):
    """The checkpoints decode TOGETHER: one beam search over the weighted mean of the members' word distributions
    (model.CaptionEnsemble).  Writes captions___ens_<n1>+<n2>+....json and a line in infer_speed.txt."""
    nums = [P_CKPT.findall(os.path.split(p)[1])[0] for p in ckpt_paths]
    mdl.reset_default_graph()
    inputs_man = inputs.InputManager(config, is_inference=True)
    try:
        return _inference_loop(inputs_man, list(ckpt_paths), None, None, ensemble_name(nums), device, weights=weights)
    finally:
        inputs_man.close()
        mdl.reset_default_graph()


def _build_ensemble(c, inputs_man, ckpt_paths, weights, device):
    members = []
    for k, path in enumerate(ckpt_paths):
        mdl.reset_default_graph()
        c.checkpoint_path = path
        m = mdl.CaptionModel(c, mode='infer', batch_ops=inputs_man.batch_infer if k == 0 else None, reuse=False,
                             name='inference (member %d)' % k, device=device)
        m.restore_model()
        members.append(mdl.CaptionEnsemble.detach(m))
    return mdl.CaptionEnsemble(members, weights)


def _ensemble_batches(ens):
    while True:
        try:
            yield ens.infer()
        except StopIteration:
            return


def _inference_loop(inputs_man, curr_ckpt_path, ckpt_dir, ckpt_file, ckpt_num, device, weights=None):
    inputs_man.enable_device_preprocess(device)
    c = inputs_man.config
    batch_size = c.batch_size_infer
    c.resume_training = False
    ensemble = isinstance(curr_ckpt_path, list)
    if ensemble:
        m_infer = _build_ensemble(c, inputs_man, curr_ckpt_path, weights, device)
    else:
        c.checkpoint_path = curr_ckpt_path
        m_infer = mdl.CaptionModel(c, mode='infer', batch_ops=inputs_man.batch_infer, reuse=False, name='inference',
                                   device=device)
        m_infer.restore_model()
    filenames = inputs_man.filenames_infer
    # required words (--infer_require_file): the table of the whole run, in input order; the model slices it per batch
    req = cdec.required_from_config(c, filenames)
    if req is not None:
        m_infer.required_table = req['required']
    # a forced prefix (--infer_prefix, --infer_prefix_file): likewise the table of the whole run
    decoder0 = m_infer.models[0].decoder if ensemble else m_infer.decoder
    pfx = cdec.prefix_from_config(c, filenames, max_steps=decoder0.max_iterations(c.infer_max_length, len(c.wtoi)))
    if pfx is not None:
        m_infer.prefix_table = pfx['prefix']
    num_batches = int(c.split_sizes['infer'] / batch_size)
    raw_outputs = dict(captions={}, attention={}, image_ids={}, beam_size=c.infer_beam_size,
                       max_caption_length=c.infer_max_length, checkpoint_path=curr_ckpt_path,
                       checkpoint_number=ckpt_num)
    coco_json = []
    groups_json = []                # diverse beam search: the group-best captions of every image
    samples_json = []               # sampling: every sample of every image, with its log-probability
    required_json = []              # required words: per image the words, met, and every non-empty bank's best caption
    prefix_json = []                # forced prefix: per image the prefix words, the cut words and the two log-probabilities
    print('INFO: Graph constructed. Starting inference.')
    start_time = time.time()
    captions = []
    # captions alone (no --save_attention_maps): the decode loops of two batches are in flight (CaptionModel.infer_pipelined)
    if ensemble:
        batches = _ensemble_batches(m_infer)
    else:
        batches = m_infer.infer_pipelined(want_attention=bool(getattr(c, 'save_attention_maps', False)))
    for step in range(num_batches):
        word_ids, attn_maps = next(batches)
        smp = getattr(m_infer, 'sample_output', None)
        captions = id_to_caption(word_ids, c, skip_unmapped=smp is not None)
        # with beam groups word_ids is group 0's best (the caption beam search of width beam / groups gives, so metrics
        # stay comparable); every group's best goes to caption_groups___N.json
        grp = getattr(m_infer, 'group_output', None)
        if grp is not None:
            G = grp['ids'].shape[1]
            grp_caps = [id_to_caption(grp['ids'][:, g], c) for g in range(G)]
        # with sampling word_ids is, per image, the sample of highest log-probability (with --infer_consensus: the one of
        # largest consensus, which every sample then carries); every sample goes to caption_samples___N.json
        if smp is not None:
            smp_caps = [id_to_caption(smp['ids'][:, k], c, skip_unmapped=True) for k in range(smp['ids'].shape[1])]
        # with required words word_ids is, per image, the best caption of the highest bank that holds one; every non-empty
        # bank's best goes to caption_required___N.json
        rqo = getattr(m_infer, 'required_output', None)
        if rqo is not None:
            rq_caps = [id_to_caption(rqo['ids'][:, k], c) for k in range(rqo['ids'].shape[1])]
        for i, f in enumerate(filenames[step * batch_size:(step + 1) * batch_size]):
            image_id = f.replace('.jpg', '')
            if '@' in image_id:
                image_id = os.path.basename(image_id)
            else:
                found = P_COCO.findall(image_id)
                if isinstance(found, list) and len(found) > 0:
                    image_id = int(found[0])
                else:
                    raise ValueError('Expected `image_id` to be list or string, saw `{}`'.format(type(found)))
            raw_outputs['captions'][f] = captions[i]
            raw_outputs['attention'][f] = attn_maps[i] if attn_maps is not None else None
            raw_outputs['image_ids'][f] = image_id
            coco_json.append(dict(image_id=image_id, caption=str(captions[i])))
            if grp is not None:
                groups_json.append(dict(image_id=image_id, captions=[
                    dict(group=g, caption=str(grp_caps[g][i]), score=float(grp['scores'][i, g]),
                         log_prob=float(grp['log_probs'][i, g])) for g in range(G)]))
            if rqo is not None:
                n_img = step * batch_size + i
                required_json.append(dict(
                    image_id=image_id, required=req['words'][n_img], dropped=req['dropped'][n_img], met=int(rqo['met'][i]),
                    bank=int(rqo['bank'][i]), captions=[
                        dict(bank=k, caption=str(rq_caps[k][i]), score=float(rqo['scores'][i, k]),
                             log_prob=float(rqo['log_probs'][i, k]))
                        for k in range(len(rq_caps)) if np.isfinite(rqo['scores'][i, k])]))
            pfo = getattr(m_infer, 'prefix_output', None)
            if pfx is not None and pfo is not None:
                n_img = step * batch_size + i
                prefix_json.append(dict(image_id=image_id, prefix=pfx['words'][n_img], cut=pfx['cut'][n_img],
                                        log_prob=float(pfo['log_prob'][i]), prefix_log_prob=float(pfo['prefix_log_prob'][i])))
            if smp is not None:
                samples_json.append(dict(image_id=image_id, captions=[
                    dict(sample=k, caption=str(smp_caps[k][i]), log_prob=float(smp['log_probs'][i, k]),
                         **(dict(consensus=float(smp['consensus'][i, k])) if 'consensus' in smp else {}))
                    for k in range(len(smp_caps))]))
    print('\nExample captions:\n{}\n'.format('\n'.join(captions[:3])))
    t = time.time() - start_time
    assert len(filenames) == len(list(set(filenames)))
    assert len(filenames) == len(coco_json)
    if c.save_attention_maps:
        with open(pjoin(c.infer_save_path, 'outputs___{}.pkl'.format(ckpt_num)), 'wb') as f:
            pickle.dump(raw_outputs, f, 2)
    with open(pjoin(c.infer_save_path, 'captions___{}.json'.format(ckpt_num)), 'w') as f:
        json.dump(coco_json, f)
    if groups_json:
        with open(pjoin(c.infer_save_path, 'caption_groups___{}.json'.format(ckpt_num)), 'w') as f:
            json.dump(groups_json, f)
    if required_json:
        with open(pjoin(c.infer_save_path, 'caption_required___{}.json'.format(ckpt_num)), 'w') as f:
            json.dump(required_json, f)
    if prefix_json:
        with open(pjoin(c.infer_save_path, 'caption_prefix___{}.json'.format(ckpt_num)), 'w') as f:
            json.dump(prefix_json, f)
    if samples_json:
        with open(pjoin(c.infer_save_path, 'caption_samples___{}.json'.format(ckpt_num)), 'w') as f:
            json.dump(samples_json, f)
    speed_file = pjoin(c.infer_save_path, 'infer_speed.txt')
    if not os.path.isfile(speed_file):
        out = ['Using GPU #: {}'.format(c.gpu), 'Inference batch size: {}'.format(c.batch_size_infer),
               'Inference beam size: {}'.format(c.infer_beam_size), '']
        with open(speed_file, 'a', newline='') as f:
            f.write('\r\n'.join(out))
    with open(speed_file, 'a', newline='') as f:
        f.write('\r\n{}'.format(len(filenames) / t))
    print('\nINFO: Inference completed. Time taken: {:4.2f} mins\n'.format(t / 60))
    return coco_json


def evaluate_model(config, curr_ckpt_path, scores_combined, valid_ppl_dict=None, test_ppl_dict=None,
                   evaluate_captions=None):
    """Runs inference for one checkpoint and, when an evaluator callable is supplied
    (annotation file, caption json) -> dict of metric scores, aggregates them like the
    reference (metric_scores.txt / .csv)."""
    c = config
    ckpt_file = os.path.split(curr_ckpt_path)[1]
    ckpt_num = int(P_CKPT.findall(ckpt_file)[0])
    coco_json = pjoin(c.infer_save_path, 'captions___{}.json'.format(ckpt_num))
    if c.run_inference:
        if not (os.path.isfile(curr_ckpt_path) or os.path.isfile(curr_ckpt_path + '.npz')
                or os.path.isfile(curr_ckpt_path + '.index')):
            print('WARNING: `{}` not found. Checkpoint skipped.'.format(ckpt_file))
            return None
        if os.path.isfile(coco_json):
            print('INFO: Found caption file `{}`. Skipping inference.'.format(os.path.basename(coco_json)))
        else:
            run_inference(config, curr_ckpt_path)
    if not c.get_metric_score or evaluate_captions is None:
        return None
    results = evaluate_captions(c.annotations_file, coco_json)
    scores_combined[ckpt_num] = results
    metrics = [m for m in ['Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'METEOR', 'ROUGE_L', 'CIDEr', 'SPICE'] if m in results]
    with open(pjoin(c.infer_save_path, 'metric_scores.txt'), 'a', newline='') as f:
        f.write('===================================\r\n%s\r\nBeam size: %d\r\n===================================\r\n'
                % (ckpt_file, c.infer_beam_size))
        f.write('\r\n'.join('{}: {:1.3f}'.format(m, results[m]) for m in metrics) + '\r\n\r\n\r\n')
    with open(pjoin(c.infer_save_path, 'metric_scores.csv'), 'a', newline='') as f:
        f.write('%d,%s\r\n' % (ckpt_num, ','.join('{:1.3f}'.format(results[m]) for m in metrics)))
    return scores_combined
