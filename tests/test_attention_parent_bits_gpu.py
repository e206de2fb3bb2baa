"""The deterministic outputs of csrc/attention.hip against the bits of the build BEFORE its region twins, mask appliers and row softmaxes
were folded into one each.  tests/golden/attention_parent.json holds, per case, one SHA-256 of the uploaded inputs and one SHA-256 per output
over its raw fp32 bytes, written on an MI355X by this module run against that build's library (VD_LIB_PATH=<that library>
VD_ATTENTION_PARENT_OUT=<file>); without the second variable every test asserts the input hash first -- a difference there says that the
inputs moved, not the kernels -- and then every output hash.  A case the file does not hold fails.

  SAN head: the CASES x {nodrop, drop} of tests/test_img_regions_ops_gpu.py, each with cnt = null, the case's counts and every count = S2;
            iqc comes from the device's own vd_img_common_forward; p, u1, dscore, dz, dqc (and iqc) are hashed.
  history:  vd_mn_attention_forward (P, hAtt) and vd_hrea_attention_forward (P, att) at the case lists of tests/test_attention_ops_gpu.py;
            vd_mn_attention_round_p / vd_hrea_attention_round_p at the shapes of tests/test_rollout_round_gpu.py, r = 0, 5 and R - 1.
  mask:     vd_img_drop_gather with a mask at the shapes of test_img_drop_gather_is_the_gather_bit_for_bit.

Outputs that go through float atomics (dwa, dba) need not repeat themselves and are not hashed: their fp64 bounds are in the modules named
above.  One module for one fixture: the entry points are tested in three modules, the record and its writer are one."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import test_attention_ops_gpu as AO
import test_img_regions_ops_gpu as RG

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'attention_parent.json')
OUT = os.environ.get('VD_ATTENTION_PARENT_OUT')
RECORD = {}                                                    # case -> {'inputs': sha, output name: sha} of this run

dev, ptr, stream = RG.dev, RG.ptr, RG.stream


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from visdial_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def golden():
    if OUT:
        return {}
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    if OUT and RECORD:                                         # how tests/golden/attention_parent.json was written (on the build before)
        with open(OUT, 'w') as f:
            json.dump(RECORD, f, indent=0, sort_keys=True)


def sha(tensors):
    """one SHA-256 over the raw bytes of the device tensors, in order; a null operand counts as its name"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(b'null' if t is None else t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def hold(golden, key, inputs, outputs):
    """inputs: the uploaded operands in a fixed order; outputs: name -> fp32 device tensor"""
    torch.cuda.synchronize()
    assert all(t.dtype == torch.float32 for t in outputs.values())
    got = dict(inputs=sha(inputs), **{name: sha([t]) for name, t in outputs.items()})
    RECORD[key] = got
    if OUT:
        return
    assert key in golden, '%s: not in %s' % (key, GOLDEN)
    want = golden[key]
    assert got['inputs'] == want['inputs'], '%s: the INPUTS of this case moved, not the kernels: nothing is said about the outputs' % key
    assert sorted(got) == sorted(want), '%s: outputs %s, recorded %s' % (key, sorted(got), sorted(want))
    moved = [name for name in sorted(outputs) if got[name] != want[name]]
    assert not moved, '%s: %s differ from the bits of the build before the fold' % (key, ', '.join(moved))


# ------------------------------------------------------------------------------------------------------------ the SAN head
@pytest.mark.parametrize("way", ['null', 'counts', 'full'])
@pytest.mark.parametrize("use_drop", [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize("shape,cnt", RG.CASES, ids=RG.IDS)
def test_san_head_keeps_the_parent_bits(lib, golden, shape, cnt, use_drop, way):
    c = RG.case(shape, cnt, use_drop)
    B, R, S2, H, Kc, N, sc = c.B, c.R, c.S2, c.H, c.Kc, c.N, c.sc
    d = RG.upload(c, cnt={'null': None, 'counts': c.cnt, 'full': np.full(B, S2, np.int32)}[way])
    forward, backward = lib.internal('vd_img_att_forward_p'), lib.internal('vd_img_att_backward_p')
    z = lambda *shape: torch.zeros(*shape, device='cuda')
    iqc, p, u1, dqc, work, dwa, dba = z(N * S2, Kc), z(N, S2), z(N, H), z(N, Kc), z(N, S2), z(Kc), z(1)
    lib.call('vd_img_common_forward', ptr(d.pre), ptr(d.m1), ptr(d.Wc), ptr(d.bc), ptr(d.qc), ptr(d.m2), ptr(iqc), N, R, S2, H, Kc, sc, stream())
    iqc_fwd = iqc.clone()
    forward(ptr(iqc), ptr(d.wa), ptr(d.ba), ptr(d.pre), ptr(d.m1), ptr(d.u0), ptr(p), ptr(u1), N, R, S2, H, Kc, sc, ptr(d.cnt), stream())
    backward(ptr(iqc), ptr(d.wa), ptr(d.pre), ptr(d.m1), ptr(d.m2), ptr(p), ptr(d.datt), ptr(dwa), ptr(dba), ptr(dqc), ptr(work), N, R, S2, H,
             Kc, sc, ptr(d.cnt), stream())
    hold(golden, 'san %s %s cnt=%s' % (shape, 'drop' if use_drop else 'nodrop', way),
         [d.pre, d.m1, d.m2, d.Wc, d.bc, d.qc, d.wa, d.ba, d.u0, d.datt, d.cnt], dict(iqc=iqc_fwd, p=p, u1=u1, dscore=work, dz=iqc, dqc=dqc))


# ------------------------------------------------------------------------------------------------------------ the history attentions
@pytest.mark.parametrize("mask_kind", ['causal', 'random'])
@pytest.mark.parametrize("B,R,H", AO.MN_CASES)
def test_mn_attention_keeps_the_parent_bits(lib, golden, B, R, H, mask_kind):
    q, h, _ = AO.mn_inputs(B, R, H)
    q, h, mask = dev(q), dev(h), dev(AO.mn_mask(B, R, H, mask_kind).astype(np.uint8))
    P, hAtt = torch.zeros(B * R, R, device='cuda'), torch.zeros(B * R, H, device='cuda')
    lib.call('vd_mn_attention_forward', ptr(q), ptr(h), ptr(mask), ptr(P), ptr(hAtt), B, R, H, stream())
    hold(golden, 'mn (%d, %d, %d) %s' % (B, R, H, mask_kind), [q, h, mask], dict(P=P, hAtt=hAtt))


@pytest.mark.parametrize("B,R,H", AO.HREA_CASES)
def test_hrea_attention_keeps_the_parent_bits(lib, golden, B, R, H):
    sq, sh, h, _ = AO.hrea_inputs(B, R, H)
    sq, sh, h = dev(sq), dev(sh), dev(h)
    P, att = torch.zeros(B * R, R, device='cuda'), torch.zeros(B * R, H, device='cuda')
    lib.call('vd_hrea_attention_forward', ptr(sq), ptr(sh), ptr(h), ptr(P), ptr(att), B, R, H, stream())
    hold(golden, 'hrea (%d, %d, %d)' % (B, R, H), [sq, sh, h], dict(P=P, att=att))


@pytest.mark.parametrize("r", [0, 5, 9])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [32, 512])
def test_round_kernels_keep_the_parent_bits(lib, golden, B, H, r):
    """R = 10; the memory query is read in place out of the per-round tensor (leading dimension R * H); dialog 0, round 5, fact 0 of the
    additive scores is an exact zero -> ReplaceZero(-inf)"""
    R, N = 10, B * 10
    rng = np.random.RandomState(100 * B + H)
    Q, Hm = AO.f32(rng, N, H) * np.float32(0.3), AO.f32(rng, N, H) * np.float32(0.3)
    sq, sh = AO.f32(rng, N), AO.f32(rng, N)
    sh[0] = -sq[5]
    Q, Hm, sq, sh = dev(Q), dev(Hm), dev(sq), dev(sh)
    z = lambda *shape: torch.zeros(*shape, device='cuda')
    P, A, Qo, Ph, Ah = z(B, R), z(B, H), z(B, H), z(B, R), z(B, H)
    lib.internal('vd_mn_attention_round_p')(ptr(Q) + r * H * 4, R * H, ptr(Hm), ptr(P), ptr(A), ptr(Qo), B, R, r, H, stream())
    lib.internal('vd_hrea_attention_round_p')(ptr(sq), ptr(sh), ptr(Hm), ptr(Ph), ptr(Ah), B, R, r, H, stream())
    hold(golden, 'round B=%d H=%d r=%d' % (B, H, r), [Q, Hm, sq, sh], dict(mn_P=P, mn_hAtt=A, mn_Qout=Qo, hrea_P=Ph, hrea_att=Ah))


# ------------------------------------------------------------------------------------------------------------ the mask applier
@pytest.mark.parametrize("H", AO.GATHER_H)
def test_img_drop_gather_keeps_the_parent_bits(lib, golden, H):
    B, R, S2 = AO.GATHER_SHAPE
    pre, m1 = AO.gather_inputs(H, True)
    pre, m1 = dev(pre), dev(m1)
    out = torch.zeros(B * R * S2, H, device='cuda')
    lib.internal('vd_img_drop_gather')(ptr(pre), ptr(m1), ptr(out), B * R, R, S2, H, 2.0, stream())
    hold(golden, 'drop_gather H=%d' % H, [pre, m1], dict(xdrop=out))
