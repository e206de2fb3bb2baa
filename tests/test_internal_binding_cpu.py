"""visdial_amd._lib.internal binds the library's internal C++ entry points (csrc/rt_core.h, csrc/common.h) from the mangled names the
built library exports.  CPU only: (a) the decoder against the (symbol, argtypes) pairs the operator suites used to carry by hand, (b) what
it refuses, (c) every declaration of the two headers against the binding of the built library, parameter by parameter, (d) the hand-written
table of the public C ABI, _lib.PROTOTYPES, against include/visdial_hip.h by type."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from visdial_amd import _lib

p, i, f, l = C.c_void_p, C.c_int, C.c_float, C.c_int64

# the hand-written bindings of tests/*_gpu.py and scripts/mb_*.py as they stood before _lib.internal replaced them (C.c_long is 64-bit)
KNOWN = [
    ('vd_img_drop_gather', '_Z18vd_img_drop_gatherPKfPKhPfiiiifP12ihipStream_t', [p, p, p, i, i, i, i, f, p]),
    ('vd_img_common_forward_p', '_Z23vd_img_common_forward_pPKfPKhS0_S0_S0_S0_S2_PfiiiiifiP12ihipStream_t', [p] * 8 + [i] * 5 + [f, i, p]),
    ('vd_img_tr_backward_p', '_Z20vd_img_tr_backward_pPKfS0_S0_S0_PKhPfiiiiifiP12ihipStream_t', [p] * 6 + [i] * 5 + [f, i, p]),
    ('vd_img_common_wgrad_p', '_Z21vd_img_common_wgrad_pPKfS0_PKhS0_PfiiiiifiP12ihipStream_t', [p] * 5 + [i] * 5 + [f, i, p]),
    ('vd_img_att_forward_p', '_Z20vd_img_att_forward_pPKfS0_S0_S0_PKhS0_PfS3_iiiiifPKiP12ihipStream_t', [p] * 8 + [i] * 5 + [f, p, p]),
    ('vd_img_att_backward_p', '_Z21vd_img_att_backward_pPfPKfS1_PKhS3_S1_S1_S_S_S_S_iiiiifPKiP12ihipStream_t', [p] * 11 + [i] * 5 + [f, p, p]),
    ('vd_clip_work_floats', '_Z19vd_clip_work_floatsv', []),
    ('vd_score_ce_p', '_Z13vd_score_ce_pPKfS0_PKiPfS3_S3_S3_iiiffP12ihipStream_t', [p] * 7 + [i, i, i, f, f, p]),
    ('vd_logsoftmax_nll_p', '_Z19vd_logsoftmax_nll_pPflliPKiS1_S_ifP12ihipStream_t', [p, l, l, i, p, p, p, i, f, p]),
    ('vd_grad_clip_scale_p', '_Z20vd_grad_clip_scale_pPKflffPfP12ihipStream_t', [p, l, f, f, p, p]),
    ('vd_clip_decay_adam_p', '_Z20vd_clip_decay_adam_pPfS_S_S_lffffffPKffP12ihipStream_t', [p] * 4 + [l] + [f] * 6 + [p, f, p]),
    ('vd_mn_attention_round_p', '_Z23vd_mn_attention_round_pPKflS0_PfS1_S1_iiiiP12ihipStream_t',
     [p, C.c_long, p, p, p, p, C.c_int, C.c_int, C.c_int, C.c_int, p]),
    ('vd_hrea_attention_round_p', '_Z25vd_hrea_attention_round_pPKfS0_S0_PfS1_iiiiP12ihipStream_t',
     [p, p, p, p, p, C.c_int, C.c_int, C.c_int, C.c_int, p]),
    ('vd_gemm_nn_live_p', '_Z17vd_gemm_nn_live_pPKflS0_lS0_PfliiiPKiiP12ihipStream_t', [p, l, p, l, p, p, l, i, i, i, p, i, p]),
    ('vd_lstm_forward_c16', '_Z19vd_lstm_forward_c16PKtlPKiPKfPtS5_PfS6_iiiP12ihipStream_t',
     [p, C.c_long, p, p, p, p, p, p, C.c_int, C.c_int, C.c_int, p]),
    ('vd_lstm_backward_c16', '_Z20vd_lstm_backward_c16PKfPtS0_S0_PfiiiP12ihipStream_t', [p, p, p, p, p, C.c_int, C.c_int, C.c_int, p]),
    ('vd_gemm_tn_acc_bf16', '_Z19vd_gemm_tn_acc_bf16PKtS0_PfliiiP12ihipStream_t', [p, p, p, C.c_long, C.c_int, C.c_int, C.c_int, p]),
    ('vd_segment_rowsum_acc_bf16', '_Z26vd_segment_rowsum_acc_bf16PKtlPKiS2_liPflP12ihipStream_t',
     [p, C.c_long, p, p, C.c_long, C.c_int, p, C.c_long, p]),
]


# ------------------------------------------------------------------------------------------------------------ a. the decoder, known pairs
@pytest.mark.parametrize("name,symbol,argtypes", KNOWN, ids=[k[0] for k in KNOWN])
def test_decoder_reproduces_the_hand_written_binding(name, symbol, argtypes):
    assert C.sizeof(C.c_long) == 8
    assert _lib.decode_argtypes(symbol, name) == argtypes


def test_decoder_widths_and_nested_pointers():
    """every builtin code by width and kind; a pointer to a pointer, a reference to a const class and substitutions of each"""
    got = _lib.decode_argtypes('_Z4vd_xijlmxyfdbahcst', 'vd_x')
    assert [C.sizeof(t) for t in got] == [4, 4, 8, 8, 8, 8, 4, 8, 1, 1, 1, 1, 2, 2]
    assert got[0] is C.c_int and got[1] is C.c_uint and got[6] is C.c_float and got[7] is C.c_double and got[8] is C.c_bool
    # S_ = Kf, S0_ = PKf, S1_ = KPKf, S2_ = PKPKf; by value S_ is a (const) float
    assert _lib.decode_argtypes('_Z4vd_xPKPKfS_S0_S2_', 'vd_x') == [p, f, p, p]
    # S_ = VdZeroSet, S0_ = K VdZeroSet, S1_ = RK VdZeroSet; PS_ appends S2_
    assert _lib.decode_argtypes('_Z4vd_xRK9VdZeroSetS1_PS_S2_Pv', 'vd_x') == [p, p, p, p, p]


# ------------------------------------------------------------------------------------------------------------ b. what the decoder refuses
@pytest.mark.parametrize("symbol,name", [
    ('_Z12vd_set_errorPKcz', 'vd_set_error'),                  # variadic
    ('_Z4vd_x10VdRowParts', 'vd_x'),                           # a class by value
    ('_Z4vd_xRK9VdZeroSetS_', 'vd_x'),                         # ... and by value through a substitution
    ('_Z4vd_xN2ns1TE', 'vd_x'),                                # a nested name
    ('_Z4vd_xI3fooEvT_', 'vd_x'),                              # a template
    ('_Z4vd_xPFivE', 'vd_x'),                                  # a pointer to a function
    ('_Z4vd_xSt6vectorIiE', 'vd_x'),                           # std::
    ('_Z4vd_xPKfS1_', 'vd_x'),                                 # a substitution that does not exist (candidates: S_, S0_)
    ('_Z4vd_xS_', 'vd_x'),
    ('_Z4vd_xiv', 'vd_x'),                                     # void by value
    ('_Z4vd_xP12ihipStr', 'vd_x'),                             # truncated
    ('_Z4vd_x', 'vd_x'),                                       # no parameter list
    ('_Z5vd_xyi', 'vd_x'),                                     # the head is not _Z<len><name>
    ('vd_x', 'vd_x'),
    ('_ZN2ns4vd_xEi', 'vd_x'),
])
def test_decoder_refuses_and_names_the_symbol(symbol, name):
    with pytest.raises(_lib.VisdialHipError) as e:
        _lib.decode_argtypes(symbol, name)
    assert symbol in str(e.value)


# ------------------------------------------------------------------------------------------------------------ c. the built library
def kind(ct):
    """(class, bytes) of a ctypes parameter type"""
    if ct in (C.c_void_p, C.c_char_p) or isinstance(ct, type(C.POINTER(C.c_int))):
        return ('ptr', 8)
    return ('float' if ct in (C.c_float, C.c_double) else 'int', C.sizeof(ct))


DECL_KIND = {'int': ('int', 4), 'int32_t': ('int', 4), 'int64_t': ('int', 8), 'long': ('int', 8), 'size_t': ('int', 8), 'uint64_t': ('int', 8),
             'float': ('float', 4), 'double': ('float', 8), 'hipStream_t': ('ptr', 8)}


def declared_kind(param):
    """(class, bytes) of one declared parameter, `type name` as the headers write it"""
    if '*' in param or '&' in param:
        return ('ptr', 8)
    words = [w for w in param.split('=')[0].split() if w != 'const']                # (a default argument is no part of the type)
    assert len(words) == 2, param                              # a builtin or typedef name and the parameter's name
    return DECL_KIND[words[0]]


def prototypes(text, ret):
    """[(return type, name, [parameters])] of the declarations `<ret> vd_name(...);` at the start of a line"""
    out = []
    for r, name, params in re.findall(r'^(%s)\s+(vd_\w+)\s*\(([^)]*)\)\s*;' % ret, text, flags=re.M):
        params = ' '.join(params.split())
        out.append((r, name, [] if params in ('', 'void') else [q.strip() for q in params.split(',')]))
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):                      # as test_host_cpu.py: it loads without a GPU
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_every_internal_declaration_binds_with_the_declared_parameter_classes(lib):
    decls = []
    for h in ('rt_core.h', 'common.h'):
        text = re.sub(r'//[^\n]*', '', open(os.path.join(ROOT, 'visdial_amd', 'csrc', h)).read())
        decls += prototypes(text, 'int|void|int64_t|size_t|bool')
    names = [d[1] for d in decls]
    assert len(set(names)) == len(names) and 'vd_score_ce_p' in names and 'vd_zero_inactive_multi' in names
    bound, refused = [], []
    for ret, name, params in decls:
        restype = C.c_int64 if ret == 'int64_t' else C.c_int
        try:
            fn = _lib.internal(name, restype)
        except _lib.VisdialHipError as e:
            assert name in str(e)
            refused.append(name)
            continue
        assert fn.symbol.startswith('_Z%d%s' % (len(name), name)) and hasattr(lib, fn.symbol), name
        assert len(fn.argtypes) == len(params), (name, fn.symbol, params)
        for ct, q in zip(fn.argtypes, params):
            assert kind(ct) == declared_kind(q), (name, q, ct)
        assert _lib.internal(name, restype) is fn              # cached
        bound.append(name)
    assert refused == ['vd_set_error']                         # variadic: the one symbol the binder must refuse
    assert len(decls) == 47 and len(bound) == len(decls) - 1   # 33 in rt_core.h + 14 in common.h as counted when this test was written
    for name, symbol, argtypes in KNOWN:                       # the library still exports what the table above was copied from
        assert name in bound and _lib.internal(name).symbol == symbol and _lib.internal(name).argtypes == argtypes, name
    # the 48th exported vd_* symbol returns a pointer, so the pattern above leaves it out: (const float*, size_t, int)
    assert [kind(t) for t in _lib.internal('vd_bf16_shadow_find', C.c_void_p).argtypes] == [('ptr', 8), ('int', 8), ('int', 4)]


def test_an_unknown_name_is_refused_by_name(lib):
    with pytest.raises(_lib.VisdialHipError, match='vd_no_such_thing_p'):
        _lib.internal('vd_no_such_thing_p')
    with pytest.raises(_lib.VisdialHipError, match='vd_score_ce'):      # a prefix of exported names is not a name
        _lib.internal('vd_score_ce_')


# ------------------------------------------------------------------------------------------------------------ d. the public table by type
RET_KIND = {'int': C.c_int, 'int64_t': C.c_int64, 'void': None, 'void*': C.c_void_p, 'const char*': C.c_char_p}


def test_public_prototypes_agree_with_the_header_by_type():
    header = open(os.path.join(ROOT, 'include', 'visdial_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    decls = prototypes(text, r'int|void\s*\*?|int64_t|const char\s*\*')
    assert len(decls) == 101 and set(d[1] for d in decls) == set(_lib.PROTOTYPES)
    for ret, name, params in decls:
        assert _lib._RESTYPE.get(name, C.c_int) is RET_KIND[re.sub(r'\s*\*', '*', ret)], (name, ret)
        table = _lib.PROTOTYPES[name]
        assert len(table) == len(params), (name, params)
        for ct, q in zip(table, params):
            assert kind(ct) == declared_kind(q), (name, q, ct)
            m = re.match(r'(?:const\s+)?(\w+)\s*\*\s*\w+$', q)                  # T* behind a POINTER(T): T of the declared width
            if isinstance(ct, type(C.POINTER(C.c_int))) and m and m.group(1) in DECL_KIND:
                assert kind(ct._type_) == DECL_KIND[m.group(1)], (name, q, ct)
            if ct is C.c_char_p:
                assert m and m.group(1) == 'char', (name, q)
