#!/usr/bin/env python
"""generate.py -- counterpart of the reference's generate.lua: load a checkpoint written by train.py, run
beam search (default) or temperature sampling with the generative decoder over the first `maxThreads`
dialogs of the val split and write vis/results/results.json-style output ({opts, data}).
Needs the real data files (or their .npz twins): question text comes from the dataset vocabulary."""
import argparse
import os

import torch

from visdial_amd import opts, utils
from visdial_amd.dataloader import Dataloader
from visdial_amd.model import Model
from visdial_amd.checkpoint import load_checkpoint, restore_weights
from visdial_amd.split_eval import check_beam_constraints, check_beam_groups


def parse_args(argv=None):
    """the command line as the `opts` of the results file; refuses top-k / nucleus truncation without -sampleWords 1 and beam groups
    that do not divide -beamSize, with a bad -beamDiversity or with -sampleWords 1, and a bad -minLen / -noRepeatNgram / -lengthPenalty
    or one of them with -sampleWords 1, -rollout 1 with -sampleWords 1 or -beamGroups > 1, and -rolloutEncoder round without -rollout 1
    -beamBatch N -host native"""
    ap = argparse.ArgumentParser(description='Test the VisDial model for generation')
    ap.add_argument('-inputImg', '--inputImg', default='data/data_img.h5')
    ap.add_argument('-inputQues', '--inputQues', default='data/visdial_data.h5')
    ap.add_argument('-inputJson', '--inputJson', default='data/visdial_params.json')
    ap.add_argument('-loadPath', '--loadPath', required=True)
    ap.add_argument('-paramOrder', '--paramOrder', default='', help="layout of the .t7 flat vector: '' | declaration | <json> (visdial_amd/t7.py resolve_order)")
    ap.add_argument('-resultPath', '--resultPath', default='vis/results')
    ap.add_argument('-beamSize', '--beamSize', type=int, default=5)
    ap.add_argument('-beamLen', '--beamLen', type=int, default=20)
    ap.add_argument('-sampleWords', '--sampleWords', type=int, default=0)
    ap.add_argument('-temperature', '--temperature', type=float, default=1.0)
    ap.add_argument('-maxThreads', '--maxThreads', type=int, default=50)
    ap.add_argument('-beamBatch', '--beamBatch', type=int, default=0,
                    help='> 0: beam search of that many dialogs at once, all on the device (0 = one dialog at a time, host bookkeeping)')
    ap.add_argument('-sampleBatch', '--sampleBatch', type=int, default=0,
                    help='> 0 (with -sampleWords 1): sample that many dialogs at once, all on the device (0 = one dialog at a time)')
    ap.add_argument('-topK', '--topK', type=int, default=0,
                    help='> 0 (with -sampleWords 1): sample among the k most likely words only (0 = off)')
    ap.add_argument('-topP', '--topP', type=float, default=1.0,
                    help='< 1 (with -sampleWords 1): sample from the smallest set of most likely words holding that share of the '
                         'probability (after -topK; 1 = off)')
    ap.add_argument('-beamGroups', '--beamGroups', type=int, default=1,
                    help='> 1: diverse beam search -- the -beamSize slots search in that many groups (it must divide -beamSize), '
                         'every round also gets `answers`, one per group (1 = off)')
    ap.add_argument('-beamDiversity', '--beamDiversity', type=float, default=0.5,
                    help='(with -beamGroups > 1) what a word costs a group for every earlier group that chose it at that step')
    ap.add_argument('-minLen', '--minLen', type=int, default=0, help='beam search: no answer of fewer than that many words (0 = off)')
    ap.add_argument('-noRepeatNgram', '--noRepeatNgram', type=int, default=0,
                    help='beam search: no n-gram of that many words occurs twice in a hypothesis (0 = off)')
    ap.add_argument('-lengthPenalty', '--lengthPenalty', type=float, default=0.0,
                    help='beam search: finished hypotheses compete on score / length^that (length = words + <END>; 0 = off)')
    ap.add_argument('-rollout', '--rollout', type=int, default=0, choices=[0, 1],
                    help='1: beam search answers every round on a history of its OWN answers to the rounds before it, not the ground '
                         'truth\'s (csrc/beam.hip R1-R6; with -beamBatch N it needs -host native; 0 = off)')
    ap.add_argument('-rolloutEncoder', '--rolloutEncoder', default='full', choices=['full', 'round'],
                    help='-rollout 1 -beamBatch N -host native: round = passes 1 .. R - 1 encode the round they answer alone instead of '
                         'the whole chunk again (csrc/rt_encoders.h forward_round); same records')
    ap.add_argument('-seed', '--seed', type=int, default=1234, help='seed of the sampling generator (numpy RandomState)')
    ap.add_argument('-gpuid', '--gpuid', type=int, default=0)
    ap.add_argument('-host', '--host', default='python', choices=['python', 'native'],
                    help="'native' drives the model-level C ABI (what lua/model.lua calls)")
    ap.add_argument('-imgRegions', '--imgRegions', type=int, default=0,
                    help='M > 0 (-host native, the two att encoders): -inputImg holds regions_<split> [n x M x C] and num_regions_<split> [n]; '
                         'every image attends its own regions only (csrc/attention.hip IR1 - IR6); from this command line, not the checkpoint')
    a = vars(ap.parse_args(argv))
    if a['imgRegions'] < 0:
        raise ValueError('-imgRegions %d must be an integer >= 0 (0 = off: one S x S grid per image)' % a['imgRegions'])
    if a['topK'] < 0 or not (0.0 < a['topP'] <= 1.0):
        raise ValueError('-topK %d must be >= 0 (0 = off) and -topP %g in (0, 1] (1 = off)' % (a['topK'], a['topP']))
    if (a['topK'] != 0 or a['topP'] != 1.0) and a['sampleWords'] != 1:
        raise ValueError('-topK / -topP truncate the sampled distribution: they need -sampleWords 1 (beam search does not truncate)')
    check_beam_groups(a['beamSize'], a['beamGroups'], a['beamDiversity'])
    if a['beamGroups'] > 1 and a['sampleWords'] == 1:
        raise ValueError('-beamGroups > 1 is diverse beam search: sampling (-sampleWords 1) has no groups')
    check_beam_constraints(a['beamSize'], a['beamLen'], a['minLen'], a['noRepeatNgram'], a['lengthPenalty'])
    if (a['minLen'] != 0 or a['noRepeatNgram'] != 0 or a['lengthPenalty'] != 0.0) and a['sampleWords'] == 1:
        raise ValueError('-minLen / -noRepeatNgram / -lengthPenalty constrain beam search: sampling (-sampleWords 1) has none')
    if a['rollout'] == 1 and a['sampleWords'] == 1:
        raise ValueError('-rollout 1 feeds the beam search\'s answers back: with -sampleWords 1 one divergent draw would cascade over the rounds')
    if a['rollout'] == 1 and a['beamGroups'] > 1:
        raise ValueError('-rollout 1 with -beamGroups %d: the choice among a round\'s groups is made on the host; a rollout over diverse beam '
                         'search is left for a follow-up' % a['beamGroups'])
    if a['rolloutEncoder'] == 'round':
        if a['rollout'] != 1:
            raise ValueError('-rolloutEncoder round encodes the later passes of a rollout one round at a time: it needs -rollout 1')
        if a['beamBatch'] <= 0:
            raise ValueError('-rolloutEncoder round belongs to the device rollout: it needs -beamBatch N (> 0); with -beamBatch 0 the host '
                             'encodes once per round and dialog')
        if a['host'] != 'native':
            raise ValueError('-rolloutEncoder round with -host python: the round pass runs in the model-level runtime only: use -host native')
    return a


def main():
    a = parse_args()
    saved = load_checkpoint(a['loadPath'])
    p = opts.derive(saved['modelParams'])                      # generate.lua:57-70
    p['gpuid'] = a['gpuid']
    p['imgRegions'], p['host'] = a['imgRegions'], a['host']
    opts.apply_img_regions(p)                                  # -imgRegions M: refusals by name, imgSpatialSize = ceil(sqrt(M))
    p.update(inputImg=a['inputImg'], inputQues=a['inputQues'], inputJson=a['inputJson'])
    # generate.lua:57-70 derives useHistory / useIm for the dataloader but NOT concatHistory (train.lua and evaluate.lua do): the history
    # of a generation run is the previous round's question + answer even for the lf-* encoders, with the default maxHistoryLen.
    # Reproduced as is (found by executing generate.lua: tests/golden/make_reference_train_golden.py).
    dl = Dataloader(seed=1234).initialize(dict(p, concatHistory=False, maxHistoryLen=60), ['val'])
    for k in ('vocabSize', 'maxQuesCount', 'maxQuesLen', 'maxAnsLen'):
        p[k] = getattr(dl, k)
    if a['host'] == 'native':
        from visdial_amd.native import NativeModel
        # the device sampler takes its truncation, the device search its groups and constraints, at creation
        model = NativeModel(dict(p, topK=a['topK'], topP=a['topP'], beamGroups=a['beamGroups'], beamDiversity=a['beamDiversity'],
                                 beamMinLen=a['minLen'], beamNoRepeat=a['noRepeatNgram'], beamLengthPenalty=a['lengthPenalty'],
                                 beamRollout=a['rollout'], rolloutEncoder=a['rolloutEncoder']))
    else:
        model = Model(p)
    restore_weights(model, saved, a['paramOrder'] or None)
    answers = model.generateAnswers(dl, 'val', dict(beamSize=a['beamSize'], beamLen=a['beamLen'],
                                                    maxThreads=a['maxThreads'], sampleWords=a['sampleWords'],
                                                    temperature=a['temperature'], beamBatch=a['beamBatch'],
                                                    sampleBatch=a['sampleBatch'], seed=a['seed'],
                                                    topK=a['topK'], topP=a['topP'], beamGroups=a['beamGroups'],
                                                    beamDiversity=a['beamDiversity'], beamMinLen=a['minLen'],
                                                    beamNoRepeat=a['noRepeatNgram'], beamLengthPenalty=a['lengthPenalty'],
                                                    rollout=a['rollout']))
    os.makedirs(a['resultPath'], exist_ok=True)
    path = os.path.join(a['resultPath'], 'results.json')
    utils.writeJSON(path, {'opts': a, 'data': answers})
    print('Writing the results to ' + path)


if __name__ == '__main__':
    main()
