#!/usr/bin/env python
"""evaluate.py -- counterpart of the reference's evaluate.lua (flags :16-30): loads a checkpoint written by train.py
(or a reference .t7), rebuilds the model from the SAVED modelParams (evaluate.lua:58-68), initialises the dataloader
on the chosen split of the REAL data files (evaluate.lua:80-81) and ranks the 100 candidate answers of every round:
-useGt 1 -> retrieve (R@1/5/10, median/mean rank, MRR), else predict.  Optionally dumps the {image_id, round_id,
ranks} records as JSON (evaluate.lua:104-107; the EvalAI submission format).  -rollout 1 ranks every round on a history of
the model's own answers to the rounds before it (visdial_amd/split_eval.py E1-E5; -rolloutHistory concat: CH1-CH6, for the encoders whose
history is the running concatenation of the dialog): the same ranks, metrics and records.  -denseAnnotations <json> adds the NDCG of the annotated rounds
(visdial_amd/dense.py; -host native: ndcg_kernel).  Without data files on disk it falls
back to synthetic VisDial-shaped batches (plumbing check only; says so)."""
import argparse
import os

from visdial_amd import opts, utils
from visdial_amd.checkpoint import load_checkpoint, restore_weights
from visdial_amd.dataloader import Dataloader, SyntheticDataloader
from visdial_amd.model import Model


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Evaluate the Visual Dialog model')
    ap.add_argument('-inputImg', '--inputImg', default='data/data_img.h5')
    ap.add_argument('-inputQues', '--inputQues', default='data/visdial_data.h5')
    ap.add_argument('-inputJson', '--inputJson', default='data/visdial_params.json')
    ap.add_argument('-loadPath', '--loadPath', required=True)
    ap.add_argument('-paramOrder', '--paramOrder', default='', help="layout of the .t7 flat vector: '' | declaration | <json> (visdial_amd/t7.py resolve_order)")
    ap.add_argument('-split', '--split', default='val')
    ap.add_argument('-useGt', '--useGt', type=int, default=1)
    ap.add_argument('-batchSize', '--batchSize', type=int, default=20)
    ap.add_argument('-gpuid', '--gpuid', type=int, default=0)
    ap.add_argument('-saveRanks', '--saveRanks', type=int, default=0)
    ap.add_argument('-saveRankPath', '--saveRankPath', default='logs/ranks.json')
    ap.add_argument('-perplexity', '--perplexity', type=int, default=0, help='also run Model:evaluate (model.lua:109-139)')
    ap.add_argument('--numThreads', type=int, default=100, help='synthetic fallback only')
    ap.add_argument('-host', '--host', default='python', choices=['python', 'native'],
                    help="'native' drives the model-level C ABI (what lua/model.lua calls)")
    ap.add_argument('-fusedLhood', '--fusedLhood', type=int, default=0, choices=[0, 1, 2],
                    help='gen decoder: score the candidates from their live (non-pad) rows only, through the fused vocabulary '
                         'projection + online log-sum-exp head (no logits buffer); 0 = the dense head; 2 = the same scores over a '
                         'prefix tree of the candidates\' tokens (a shared beginning is computed once; needs -host native)')
    ap.add_argument('-optionCache', '--optionCache', type=int, default=0,
                    help='disc decoder: keep the encoding of every distinct candidate answer on the device while the split is ranked and run '
                         'the option LSTM over the answers not seen before only (0 = off, 1 = on, larger = capacity in rows)')
    ap.add_argument('-rollout', '--rollout', type=int, default=0, choices=[0, 1],
                    help='rank every round on a history of the model\'s OWN answers to the rounds before it instead of the ground truth\'s: '
                         'disc feeds the rank-1 candidate back (-host native: on the device, -host python: a host loop of one retrieval '
                         'per round), gen the beam search\'s answer, as generate.py -rollout 1 (needs -host native)')
    ap.add_argument('-beamSize', '--beamSize', type=int, default=5, help='-rollout 1, gen decoder: the beam search that answers')
    ap.add_argument('-beamLen', '--beamLen', type=int, default=20)
    ap.add_argument('-minLen', '--minLen', type=int, default=0, help='-rollout 1, gen decoder: as generate.py')
    ap.add_argument('-noRepeatNgram', '--noRepeatNgram', type=int, default=0)
    ap.add_argument('-lengthPenalty', '--lengthPenalty', type=float, default=0.0)
    ap.add_argument('-rolloutEncoder', '--rolloutEncoder', default='full', choices=['full', 'round'],
                    help='-rollout 1 -host native: round = passes 1 .. R - 1 of the device rollout encode the round they rank alone instead '
                         'of the whole batch again (csrc/rt_encoders.h forward_round; for gen: the beam-search rollout); same records')
    ap.add_argument('-rolloutHistory', '--rolloutHistory', default='row', choices=['row', 'concat'],
                    help='-rollout 1: row = every history row holds one round (E4); concat = the encoders that read the running concatenation '
                         'of the dialog (lf-ques-hist, lf-ques-im-hist, lf-att-ques-im-hist) roll out by the concatenation rule '
                         '(visdial_amd/split_eval.py CH1-CH6): row r + 1 = row r, <END>, the question, the answer, cut at the end where it does not fit')
    ap.add_argument('-denseAnnotations', '--denseAnnotations', default='',
                    help='a file of dense relevance annotations (VisDial v1.0: a JSON list of {image_id, round_id, gt_relevance}): also print the '
                         'NDCG of the annotated rounds of the split (csrc/loss.hip DT2; -host native: on the device) and add it to their records')
    ap.add_argument('-imgRegions', '--imgRegions', type=int, default=0,
                    help='M > 0 (-host native, the two att encoders): -inputImg holds regions_<split> [n x M x C] and num_regions_<split> [n]; '
                         'every image attends its own regions only (csrc/attention.hip IR1 - IR6).  A property of the data: it comes '
                         'from this command line, not from the checkpoint.  0 = off')
    a = ap.parse_args(argv)
    if a.imgRegions < 0:
        raise SystemExit('-imgRegions %d must be an integer >= 0 (0 = off: one S x S grid per image)' % a.imgRegions)
    if a.rolloutHistory == 'concat' and not a.rollout:
        raise SystemExit('-rolloutHistory concat is the history rule of a rollout: it needs -rollout 1')
    if a.rolloutEncoder == 'round':
        if not a.rollout:
            raise SystemExit('-rolloutEncoder round encodes the later passes of a rollout one round at a time: it needs -rollout 1')
        if a.host != 'native':
            raise SystemExit('-rolloutEncoder round with -host python: the round pass runs in the model-level runtime only: use -host native')
    return a


def check_rollout(a, p):
    """what -rollout 1 cannot be combined with, for the derived model params `p`: each refusal names its flag"""
    if not a.rollout:
        return
    if a.optionCache:
        raise SystemExit('-rollout 1 with -optionCache: a cached batch carries only the candidates the cache did not hold, and the rollout '
                         'reads a picked candidate\'s tokens from the batch; combining the two is left for a follow-up')
    if a.perplexity:
        raise SystemExit('-rollout 1 with -perplexity 1: perplexity is defined on the ground-truth history; run it separately')
    concat = getattr(a, 'rolloutHistory', 'row') == 'concat'
    if p.get('useHistory') and p.get('concatHistory') and not concat:
        raise SystemExit("-rollout 1 with encoder '%s': it reads the running concatenation of the rounds (concatHistory), and the rollout's "
                         "rule describes the per-round history row only; -rolloutHistory concat lifts the refusal: it rolls out by the "
                         "concatenation rule" % p['encoder'])
    if concat and p.get('useHistory') and not p.get('concatHistory'):
        raise SystemExit("-rolloutHistory concat with encoder '%s': its history is one row per round, not the running concatenation; the "
                         "concatenation rule is for lf-ques-hist, lf-ques-im-hist and lf-att-ques-im-hist" % p['encoder'])
    if p['decoder'] == 'gen' and a.host != 'native':
        raise SystemExit('-rollout 1 with a generative model feeds the beam search\'s answers back on the device: add -host native')


def main(argv=None):
    a = parse_args(argv)
    saved = load_checkpoint(a.loadPath)
    p = opts.derive(saved['modelParams'])                    # sets useHistory / useIm / concatHistory (evaluate.lua:69-75)
    p['gpuid'], p['batchSize'], p['useGt'] = a.gpuid, a.batchSize, bool(a.useGt)
    p['imgRegions'], p['host'] = a.imgRegions, a.host
    try:
        opts.apply_img_regions(p)                            # -imgRegions M: refusals by name, imgSpatialSize = ceil(sqrt(M))
    except ValueError as e:
        raise SystemExit(str(e))
    if a.fusedLhood and p['decoder'] != 'gen':
        raise SystemExit('-fusedLhood %d: the live-row log-likelihood head is only for a generative model' % a.fusedLhood)
    if a.fusedLhood == 2 and a.host != 'native':
        raise SystemExit('-fusedLhood 2: the prefix-tree head runs in the model-level runtime only: add -host native')
    p['fusedLhood'] = a.fusedLhood
    if a.optionCache and p['decoder'] != 'disc':
        raise SystemExit('-optionCache: the answer-encoding cache is only for a discriminative model')
    p['optionCache'] = a.optionCache
    check_rollout(a, p)
    p['rollout'] = a.rollout
    p['rolloutEncoder'] = a.rolloutEncoder
    concat = bool(a.rollout and a.rolloutHistory == 'concat' and p.get('useHistory'))     # (no history: ignored, like the other rollout flags)
    p['rolloutHistory'] = 'concat' if concat else 'row'
    p.update(inputImg=a.inputImg, inputQues=a.inputQues, inputJson=a.inputJson)
    have = lambda f: os.path.exists(f) or os.path.exists(f[:-3] + '.npz')
    if os.path.exists(a.inputJson) and have(a.inputQues):
        try:
            dl = Dataloader(seed=1234).initialize(p, [a.split])                  # evaluate.lua:80-81
        except ValueError as e:                                                  # (-imgRegions: a dataset that does not hold M regions)
            raise SystemExit(str(e))
        for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen', 'numOptions'):
            p[k] = getattr(dl, k)
    else:
        print('no dataset at %s: ranking SYNTHETIC batches (plumbing check, the metrics mean nothing)' % a.inputQues)
        dl = SyntheticDataloader(p, seed=4321, num_threads=a.numThreads)
    if concat:                                                # CH3's <END>: the host loop's and, for -host native, the device rollout's
        w2i = getattr(dl, 'word2ind', None)
        p['rolloutConcatEnd'] = int(w2i['<END>'] if w2i else dl.endToken)
    if a.rollout and p['decoder'] == 'gen':
        # the device search takes its knobs when the model is created; the answers are the ones generate.py -rollout 1 -beamBatch N writes
        w2i = getattr(dl, 'word2ind', None)
        start, end = (w2i['<START>'], w2i['<END>']) if w2i else (dl.startToken, dl.endToken)
        p.update(beamRollout=1, beamMinLen=a.minLen, beamNoRepeat=a.noRepeatNgram, beamLengthPenalty=a.lengthPenalty,
                 rolloutBeam=dict(beamSize=a.beamSize, beamLen=a.beamLen, startToken=start, endToken=end))
    elif a.rollout and a.host == 'native':
        p['retrieveRollout'] = 1
    if a.host == 'native':
        from visdial_amd.native import NativeModel
        model = NativeModel(p)
    else:
        try:
            model = Model(p)
        except ValueError as e:
            raise SystemExit(str(e))
    restore_weights(model, saved, a.paramOrder or None)          # evaluate.lua:91
    if a.denseAnnotations:                                       # NDCG reads the final scores: every decoder, head, cache and rollout
        from visdial_amd.dense import load_dense_annotations
        try:
            model.denseAnnotations = load_dense_annotations(a.denseAnnotations)
        except (OSError, ValueError) as e:
            raise SystemExit('-denseAnnotations: %s' % e)
    print('Evaluating..')
    if a.perplexity:
        model.evaluate(dl, a.split)
    if a.useGt:
        metrics, records = model.retrieve(dl, a.split)
    else:
        records = model.predict(dl, a.split)
    if a.fusedLhood == 2:
        st = model.lhoodTreeStats
        print('fusedLhood 2: %d nodes for %d live rows (%.3f); the candidate recurrence ran %d of %d (step, candidate) rows (%.1f %%)'
              % (st['nodes'], st['live'], st['nodes'] / max(st['live'], 1), st['executed'], st['total'],
                 100.0 * st['executed'] / max(st['total'], 1)))
    if a.rollout:
        print('rollout: %d of %d history rows differ from the ground truth\'s' % model.rolloutRows)
        if concat:
            print('rolloutHistory concat: %d generated history rows were cut to the history\'s width (CH4)' % model.rolloutCut)
    if a.optionCache:
        ex, tot = model.optionCacheRows
        print('optionCache: the option LSTM ran %d of %d candidate rows (%.1f %%)' % (ex, tot, 100.0 * ex / max(tot, 1)))
    if a.saveRanks:
        print('Writing ranks to %s' % a.saveRankPath)
        os.makedirs(os.path.dirname(os.path.abspath(a.saveRankPath)), exist_ok=True)
        utils.writeJSON(a.saveRankPath, records)


if __name__ == '__main__':
    main()
