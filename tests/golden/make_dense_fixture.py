"""Writes tests/golden/dense/val_dense_annotations.json and train_dense_sample.json: dense relevance annotations for the image ids of the
committed prepro fixture (tests/golden/prepro: val images 2001-2004, train images 1001-1005, R = 10 rounds, O = 100 candidates), in the
format of the public VisDial v1.0 dataset's description -- a JSON list of {"image_id", "round_id" (1-based), "gt_relevance": [O floats]};
the train sample says "relevance" instead.  The real files are on no machine this project is developed on, so the values are drawn here
with a fixed seed: relevances are multiples of 0.2 (the public annotations average a few annotators' votes), mostly 0.

The cases the tests lean on:
  val   2001 round 3: ties in relevance (many 0.4 / 0.2 entries)      2002 round 7: k = O, every candidate relevant
        2003 round 1: k = 1                                           2004 round 10: k = 0, no relevant candidate
        + one annotation of image 9999, which is in no split
  train 1001 round 2, 1002 round 5, 1004 round 9 (ties, k = 1, random); dialogs 1003 and 1005 have no annotation

    python tests/golden/make_dense_fixture.py
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
O = 100


def sparse(rng, k):
    """k relevant candidates with relevances from {0.2, .., 1.0}, the rest 0"""
    rel = np.zeros(O)
    rel[rng.choice(O, size=k, replace=False)] = rng.randint(1, 6, size=k) / 5.0
    return rel


def main():
    rng = np.random.RandomState(20181)
    ties = np.zeros(O)
    ties[rng.choice(O, size=30, replace=False)] = np.repeat([0.4, 0.2, 1.0], 10)
    one = np.zeros(O)
    one[37] = 0.6
    val = [dict(image_id=2001, round_id=3, gt_relevance=ties),
           dict(image_id=2002, round_id=7, gt_relevance=rng.randint(1, 6, size=O) / 5.0),
           dict(image_id=2003, round_id=1, gt_relevance=one),
           dict(image_id=2004, round_id=10, gt_relevance=np.zeros(O)),
           dict(image_id=9999, round_id=4, gt_relevance=sparse(rng, 12))]
    train_ties = np.zeros(O)
    train_ties[rng.choice(O, size=20, replace=False)] = 0.5
    one2 = np.zeros(O)
    one2[3] = 1.0
    train = [dict(image_id=1001, round_id=2, relevance=train_ties),
             dict(image_id=1002, round_id=5, relevance=one2),
             dict(image_id=1004, round_id=9, relevance=sparse(rng, 9))]
    os.makedirs(os.path.join(HERE, 'dense'), exist_ok=True)
    for name, entries in (('val_dense_annotations.json', val), ('train_dense_sample.json', train)):
        for e in entries:
            key = 'gt_relevance' if 'gt_relevance' in e else 'relevance'
            e[key] = [round(float(v), 1) for v in e[key]]
        with open(os.path.join(HERE, 'dense', name), 'w') as f:
            json.dump(entries, f)
            f.write('\n')


if __name__ == '__main__':
    main()
