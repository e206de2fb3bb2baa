"""The split-level loops of visdial_amd/split_eval.py (evaluate / retrieve / predict / generateAnswers) against what they returned,
printed, tallied and asked of their host when tests/golden/split_loops.json was recorded: tests/golden/make_split_loops_fixture.py
drives them over a numpy stand-in host with no device and no library, and everything is compared exactly -- the ordered list of host
calls too, so a change that adds or drops device work fails here.  The fixture is not regenerated from later code."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope="module")
def replay():
    spec = importlib.util.spec_from_file_location('make_split_loops_fixture', os.path.join(GOLDEN, 'make_split_loops_fixture.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    with open(os.path.join(GOLDEN, 'split_loops.json')) as f:
        want = json.load(f)
    return json.loads(json.dumps(make.run_cases())), want


def test_every_case_replays_exactly(replay):
    got, want = replay
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        for key in sorted(want[name]):
            assert got[name].get(key) == want[name][key], (name, key)
        assert got[name] == want[name], name


def test_the_fixture_reaches_the_branches_it_is_there_for(replay):
    _, want = replay
    calls = lambda name, method: sum(c[0] == method for c in want[name]['calls'])
    assert all('result' in c or 'error' in c for c in want.values())
    for method in ('retrieve', 'predict'):
        # plain: one retrieval per batch, the last batch ragged; a rollout: R per batch, on the untrimmed history
        assert calls(method + ' plain', 'retrieveBatch') == 2 and calls(method + ' rollout', 'retrieveBatch') == 6
        assert want[method + ' rollout']['rolloutRows'][1] == 9 and want[method + ' rollout']['rolloutRows'][0] >= 1
        assert want[method + ' rollout concat']['rolloutCut'] >= 1                   # CH4 cut a row
        assert want[method + ' rollout no history']['rolloutRows'] == [0, 0] and calls(method + ' rollout no history', 'retrieveBatch') == 2
        assert want[method + ' optionCache']['optionCacheRows'][1] == 45 and want[method + ' gen lhood tree']['lhoodTreeStats']['total'] == 45
        rows = want[method + ' dense']['ndcgRows']
        assert rows[0][1] >= 0 and rows[1] == [-1.0, -2.0, -2.0] and rows[2][2] >= 0 and 'NDCG: ' in want[method + ' dense']['stdout']
    assert [r['round_id'] for r in want['predict test dense']['result']] == [3, 2, 3]
    assert [c[0] for c in want['evaluate gen']['calls']] == ['forwardBackward'] * 2
    assert calls('generate beamBatch 2', '_gen_beam') == 2 and calls('generate beamBatch 2', '_gen_step') == 0
    assert calls('generate row beamBatch 0', '_gen_encode') == 3 and calls('generate row rollout', '_gen_encode') == 9
    assert want['generate row rollout']['result'] != want['generate row beamBatch 0']['result']
    assert calls('generate nohist rollout', '_gen_encode') == 3
    assert all(len(e['answers']) == 2 for d in want['generate beamGroups 2']['result'] for e in d['dialog'])
    assert want['generate beamGroups 2 beamBatch 2']['result'] == want['generate beamGroups 2']['result']
    assert want['generate constraints']['result'] != want['generate row beamBatch 0']['result']
    assert want['generate constraints beamBatch 2']['result'] == want['generate constraints']['result']
    assert calls('generate sampleWords sampleBatch 2', '_gen_sample') == 2
    assert want['generate sampleWords topK topP']['result'] != want['generate sampleWords']['result']
    refused = [n for n in want if ' refuses: ' in n]
    assert len(refused) == 25 and all('error' in want[n] and 'result' not in want[n] for n in refused)
    # a refusal of generateAnswers comes before any device work: at most the question whether the device can do it was asked
    assert all(c[0] in ('_sample_truncation', '_beam_grouping', '_beam_constraints', '_beam_rollout')
               for n in refused for c in want[n]['calls'])
