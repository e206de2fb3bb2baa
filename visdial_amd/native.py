"""`NativeModel` -- the training / retrieval step of any encoder x decoder plug-in pair driven entirely through the
MODEL-LEVEL C ABI (include/visdial_hip.h, csrc/runtime.hip): the same handful of calls a LuaJIT `model.lua` proxy
makes.  Python only converts numpy batches to host pointers; streams, the skewed LSTM wavefront,
the length sort, workspaces and launch order live in the library.  Same method names as visdial_amd.model.Model /
the reference's Model (model.lua): trainIteration, forwardBackward, update, retrieveBatch."""
import ctypes as C

import numpy as np

from . import _lib
from .split_eval import SplitEval, rollout_answered_history

call = _lib.call


def _text(v):
    return None if v is None else str(v)


def _int0(v):
    return int(v or 0)


SWITCHES = (
    # params key, variable, text of the params value, type and default of the resolved value, decoder it applies to (None = both)
    ('optionCache', 'VD_OPTION_CACHE', lambda v: str(_int0(v)), _int0, 0, None),          # 0 = off, 1 = on, larger = capacity in rows
    ('fusedLhood', 'VD_LHOOD_TREE', lambda v: '1' if _int0(v) == 2 else '0', _int0, 0, None),   # 2 = retrieval over a prefix tree
    ('topK', 'VD_SAMPLE_TOPK', _text, int, 0, 'gen'),                                     # truncation inside vd_model_sample
    ('topP', 'VD_SAMPLE_TOPP', _text, float, 1.0, 'gen'),
    ('beamGroups', 'VD_BEAM_GROUPS', _text, int, 1, 'gen'),                               # diverse search inside vd_model_beam_search
    ('beamDiversity', 'VD_BEAM_DIVERSITY', _text, float, 0.5, None),                      # (kept for disc too: only looked at when G > 1)
    ('beamMinLen', 'VD_BEAM_MIN_LEN', _text, int, 0, 'gen'),                              # the constraints of vd_model_beam_search
    ('beamNoRepeat', 'VD_BEAM_NO_REPEAT', _text, int, 0, 'gen'),
    ('beamLengthPenalty', 'VD_BEAM_LENGTH_PENALTY', _text, float, 0.0, 'gen'),
    ('beamRollout', 'VD_BEAM_ROLLOUT', _text, int, 0, 'gen'),                             # the search rolls its answers into the history
    ('retrieveRollout', 'VD_RETRIEVE_ROLLOUT', _text, int, 0, 'disc'),                    # vd_model_retrieve rolls its picks into it
    ('rolloutEncoder', 'VD_ROLLOUT_ENCODER', _text, str, 'full', None),                   # 'round': passes 1 .. R - 1 encode one round
    ('rolloutConcatEnd', 'VD_ROLLOUT_CONCAT_END', _text, int, 0, None),                   # the <END> id: a rollout writes concatenated rows
)
"""The switches the library reads from the environment inside vd_model_create (csrc/rt_switches.h; the Lua host sets the same variables).
NativeModel sets every row's variable to the text of its params value -- unset where that is None: a params without the key creates the
model with the variable unset -- creates the model and puts the previous environment back, also after a failed create, so two models of
one process can differ.  Python validates nothing: the values go through as written and the library is the one that refuses.  What the
model was created with stays in `NativeModel._knobs` (the default for a row of the other decoder, which the library does not read);
generateAnswers checks what it is asked for against it.  rolloutConcatEnd (VD_ROLLOUT_CONCAT_END) is the <END> id of a rollout on a
concatenated history (split_eval.py CH1-CH6): evaluate.py -rolloutHistory concat fills it from the loader, and `retrieve_rollout_batch`
refuses a device rollout whose params rolloutHistory does not agree with what the model was created with."""

TRAIN_SWITCHES = (
    # rows of the same type, chained behind SWITCHES: the knobs of a training step (loss.hip LS1-LS4; elementwise.hip GC1-GC3, WD1)
    ('labelSmoothing', 'VD_LABEL_SMOOTHING', _text, float, 0.0, None),                    # vd_model_forward_backward(m, 0): soft targets
    ('gradClipNorm', 'VD_GRAD_CLIP_NORM', _text, float, 0.0, None),                       # vd_model_update: global-norm clip
    ('weightDecay', 'VD_WEIGHT_DECAY', _text, float, 0.0, None),                          # vd_model_update: decoupled weight decay
)

DENSE_SWITCHES = (
    # rows of the same type, chained behind TRAIN_SWITCHES: dense-annotation fine-tuning (loss.hip DT1-DT5)
    ('denseMix', 'VD_DENSE_MIX', _text, float, 0.0, None),                                # weight of a round without an annotation in a dense step
)
"""What a dense step adds to the environment.  The relevance matrix itself is no switch: it is a batch attachment, `attach_dense_relevance`
(vd_model_set_tensor '@dense_relevance') behind an upload, and `ndcg_rows` (vd_model_get_tensor '@ndcg') reads the NDCG of the scores.
Neither is the choice of the rows a dense step executes: `attach_dense_relevance(rel, live=True)` attaches the matrix under the name
'@dense_relevance_live' (params denseRows = 'live' makes `upload` do so for a dense batch)."""

ALL_SWITCHES = SWITCHES + TRAIN_SWITCHES + DENSE_SWITCHES


class _DevArray(object):
    """a raw device pointer as something torch.as_tensor understands (plumbing for torch.distributed only)"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': '<f4', 'data': (ptr, False), 'version': 2}


class _Optims(object):
    """`model.optims` of the reference (model.lua:58-63): only learningRate is host-visible; the Adam moments live in
    the library"""

    def __init__(self, model):
        self._m = model

    def _lr(self, value=None):
        v = C.c_double(0.0 if value is None else float(value))
        call("vd_model_learning_rate", self._m.h, C.byref(v), 0 if value is None else 1)
        return float(v.value)

    def __getitem__(self, k):
        if k != 'learningRate':
            raise KeyError(k)
        return self._lr()

    def __setitem__(self, k, v):
        if k != 'learningRate':
            raise KeyError(k)
        self._lr(v)

    def keys(self):
        return ['learningRate']


class NativeModel(SplitEval):
    def __init__(self, params, init_seed=1234, dist_group=None, library_comm=False):
        """library_comm=True: the gradient all-reduce is the library's own (vd_comm_init has been called in this process,
        visdial_amd.parallel.init_library_comm): RCCL behind the ABI, no Python in the reduce path.  dist_group: the
        older host-side path over torch.distributed (kept as the gloo test vehicle and for the operator-level host)."""
        p = params
        self.dist_group = dist_group
        self.library_comm = bool(library_comm)
        self._dW = None
        mp = _lib.ModelParams(
            vocabSize=p['vocabSize'], embedSize=p['embedSize'], rnnHiddenSize=p['rnnHiddenSize'],
            imgFeatureSize=p.get('imgFeatureSize', 0), imgSpatialSize=p.get('imgSpatialSize', 1),
            commonEmbeddingSize=p.get('commonEmbeddingSize', 512), numAttentionLayers=int(p.get('numAttentionLayers', 1) or 1),
            maxQuesCount=p['maxQuesCount'], numOptions=p.get('numOptions', 100),
            learningRate=p.get('learningRate', 1e-3), lrDecayRate=p.get('lrDecayRate', 0.9997592083),
            minLRate=p.get('minLRate', 5e-5), seed=int(p.get('seed', 1234)) + 7919 * int(p.get('rank', 0)),
            lstmBf16={'fp32': 0, 'bf16': 1, 'split9': 9, 'split6': 6, 'split3': 3}[p.get('lstmPrecision', 'split9')], useStreams=int(p.get('useStreams', 1)),
            numLayers=int(p.get('numLayers', 2)), imgEmbedSize=int(p.get('imgEmbedSize', 300)),
            dropout=float(p.get('dropout', 0.5)))
        self.params = p
        h = C.c_void_p()
        import os
        switches = {var: text(p.get(key)) for key, var, text, _, _, _ in ALL_SWITCHES}

        def put(values):
            for k, v in values.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        prev = {k: os.environ.get(k) for k in switches}
        try:
            put(switches)
            call("vd_model_create", C.byref(mp), p['encoder'].encode(), p['decoder'].encode(), C.byref(h))
        finally:
            put(prev)
        self._knobs = {key: default if p.get(key) is None or decoder not in (None, p['decoder']) else conv(p[key])
                       for key, _, _, conv, default, decoder in ALL_SWITCHES}
        self.h = h
        lib = _lib.load()
        self.tensors = []
        name = C.create_string_buffer(64)
        off, r, c = C.c_int64(), C.c_int64(), C.c_int64()
        for i in range(lib.vd_model_num_tensors(h)):
            call("vd_model_tensor_info", h, i, name, C.byref(off), C.byref(r), C.byref(c))
            self.tensors.append((name.value.decode(), int(off.value), int(r.value), int(c.value)))
        call("vd_model_init_params", h, int(init_seed))
        self._keep = None
        self._next_batch, self._next_src = None, None
        self.runningLoss = 0.0
        self._W = None
        self.optims = _Optims(self)

    def close(self):
        if self.h:
            _lib.load().vd_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def _shape(self, name, r, c):
        return (c,) if name.endswith('.b') else (r, c)

    def set_parameters_dict(self, d):
        for name, _, r, c in self.tensors:
            a = np.ascontiguousarray(d[name], dtype=np.float32)
            assert a.size == r * c, name
            call("vd_model_set_tensor", self.h, name.encode(), a.ctypes.data, a.size)

    def _get(self, which):
        out = {}
        for name, _, r, c in self.tensors:
            a = np.empty(self._shape(name, r, c), np.float32)
            call("vd_model_get_tensor", self.h, name.encode(), which, a.ctypes.data, a.size)
            out[name] = a
        return out

    def get_parameters_dict(self):
        return self._get(0)

    def get_gradients_dict(self):
        return self._get(1)

    @property
    def wrapperW(self):
        """the flat parameter vector (device tensor aliasing the library's buffer; same aligned layout as
        visdial_amd.model.Model.wrapperW, so `.pt` checkpoints are interchangeable between the two hosts)"""
        if self._W is None:
            import torch
            ptrs = [C.c_void_p() for _ in range(4)]
            call("vd_model_flat_pointers", self.h, *[C.byref(x) for x in ptrs])
            n = int(_lib.load().vd_model_flat_size(self.h))
            self._W = torch.as_tensor(_DevArray(ptrs[0].value, n), device='cuda')
        self.synchronize()
        return self._W

    def _entries(self):
        kind = lambda n: 'embed' if n == 'embed' else ('lstm' if n.split('.')[0].rstrip('0123456789') in
                                                        ('hist', 'ques', 'opt', 'dec', 'dialog') else 'lin') + \
            ('_w' if n.endswith('.W') else '_b')
        return [(n, self._shape(n, r, c), kind(n)) for n, _, r, c in self.tensors]

    def load_flat_parameters(self, modelW):
        """`model.wrapperW:copy(savedModel.modelW)` for a flat vector in the REFERENCE's getParameters() layout
        (see visdial_amd.model.Model.load_flat_parameters).  Goes through vd_model_set_tensor, which also empties the answer-encoding
        cache; a host that writes through `wrapperW` instead must call training(True) afterwards."""
        from . import t7
        self.set_parameters_dict(t7.flat_to_named(np.asarray(modelW), self._entries(), self.params['encoder']))

    def flat_parameters(self):
        from . import t7
        return t7.named_to_flat(self.get_parameters_dict(), self._entries(), self.params['encoder'])

    def training(self, on=True):
        call("vd_model_set_training", self.h, int(on))

    def set_dropout_masks(self, masks):
        call("vd_model_set_dropout_mask", self.h, None, None, 0)
        for k, v in (masks or {}).items():
            a = np.ascontiguousarray(np.asarray(v) != 0, dtype=np.uint8).reshape(-1)
            call("vd_model_set_dropout_mask", self.h, k.encode(), a.ctypes.data, a.size)

    # ------------------------------------------------------------------ step
    def upload(self, batch):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        keep = []                                   # host buffers stay alive until the call returns

        def ptr(a):
            keep.append(a)
            return a.ctypes.data
        q = i32(batch['ques_fwd'].reshape(-1, batch['ques_fwd'].shape[2]))
        hb = _lib.Batch(B=batch['ques_fwd'].shape[0], Tq=q.shape[1], ques_fwd=ptr(q))
        if 'hist' in batch:
            h = i32(batch['hist'].reshape(-1, batch['hist'].shape[2]))
            hb.Th, hb.hist = h.shape[1], ptr(h)
        if 'img_feat' in batch:
            hb.img_feat = ptr(np.ascontiguousarray(batch['img_feat'], dtype=np.float32))
        if 'options' in batch:
            o = i32(batch['options'])
            hb.To, hb.options = o.shape[-1], ptr(o)
        if 'answer_ind' in batch:
            hb.answer_ind = ptr(i32(batch['answer_ind'].reshape(-1)))
        if 'answer_in' in batch:
            a = i32(batch['answer_in'])
            hb.Ta, hb.answer_in, hb.answer_out = a.shape[-1], ptr(a), ptr(i32(batch['answer_out']))
        if 'option_in' in batch:
            a = i32(batch['option_in'])
            hb.To, hb.option_in, hb.option_out = a.shape[-1], ptr(a), ptr(i32(batch['option_out']))
        call("vd_model_upload_batch", self.h, C.byref(hb))      # host buffers are consumed before it returns
        self._N = batch['ques_fwd'].shape[0] * batch['ques_fwd'].shape[1]
        if batch.get('dense_relevance') is not None:            # a dense batch (dataloader.getDenseTrainBatch) trains on its matrix
            self.attach_dense_relevance(batch['dense_relevance'], live=self.params.get('denseRows', 'all') == 'live')
        if batch.get('img_regions') is not None:                # detector regions: every image attends its own first count rows
            self.attach_img_regions(batch['img_regions'])
        # non-pad target tokens of THIS batch: the gen loss EMA divides by it (model.lua:76-85)
        self._numTokens = float((np.asarray(batch['answer_out']) > 0).sum()) if 'answer_out' in batch else 0.0
        # whatever was prefetched for trainIteration has just been replaced (evaluate / retrieve / predict / generate
        # between two training steps): the next trainIteration must fetch its own batch
        self._keep = None

    def attach_dense_relevance(self, rel, live=False):
        """attach the relevance matrix [N x O] (dense.relevance_matrix: DT1) to the batch uploaded last: a training step of a disc model
        then takes the dense target (DT3-DT4), and `ndcg_rows` ranks with it.  The library validates it and refuses by name.
        live=True attaches it as '@dense_relevance_live' (DL1-DL5): the same matrix and the same step, with the option recurrence and its
        gradients run over the candidate rows of the rounds of weight > 0 only (`option_rows` reports them).  An attachment replaces the
        one before it on the same upload."""
        a = np.ascontiguousarray(rel, dtype=np.float32)
        call("vd_model_set_tensor", self.h, b"@dense_relevance_live" if live else b"@dense_relevance", a.ctypes.data, a.size)

    def attach_img_regions(self, counts):
        """attach the number of live regions of every image [B] (integers in 1 .. imgSpatialSize^2) to the batch uploaded last
        (vd_model_set_tensor '@img_regions'; csrc/attention.hip IR1 - IR6): the image attention of every pass over that upload -- training
        step, retrieval, generation, rollouts -- looks at the first counts[b] regions of image b and at nothing else.  The hidden rows of
        the uploaded img_feat must be finite (the loaders write zeros).  The library validates the counts and refuses by name; the next
        upload clears them."""
        a = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.float32)
        call("vd_model_set_tensor", self.h, b"@img_regions", a.ctypes.data, a.size)

    def ndcg_rows(self):
        """NDCG [N] (float64) of the scores of the last forward / retrieval of the current batch under its attached relevance matrix
        (ndcg_kernel; DT2): -1 = no relevant candidate, -2 = not annotated.  The call returns the kernel's doubles bit for bit in 2 N floats."""
        out = np.empty(int(self._N), np.float64)
        call("vd_model_get_tensor", self.h, b"@ndcg", 0, out.ctypes.data, 2 * out.size)
        return out

    def _ndcg_of_batch(self, batch, rel):
        self.attach_dense_relevance(rel)
        return self.ndcg_rows()

    def _train_batch(self, dataloader):
        """the next training batch: params denseAnnotations (a file of dense annotations) draws annotated dialogs with their matrix"""
        path = self.params.get('denseAnnotations')
        if not path:
            return dataloader.getTrainBatch(self.params)
        if getattr(self, '_dense', None) is None or self._dense[0] != path:
            from .dense import load_dense_annotations
            self._dense = (path, load_dense_annotations(path))
        return dataloader.getDenseTrainBatch(self.params, self._dense[1])

    def forwardBackward(self, batch=None, onlyForward=False, deferLoss=False):
        if batch is not None:
            self.upload(batch)
        call("vd_model_forward_backward", self.h, int(onlyForward))
        return self.loss if deferLoss else self.loss()

    def loss(self):
        v = C.c_float()
        call("vd_model_loss", self.h, C.byref(v))
        return float(v.value)

    def _dp_active(self):
        import os
        if self.dist_group is None:
            return False
        import torch.distributed as dist
        return dist.get_world_size(self.dist_group) > 1 or os.environ.get('VD_FORCE_ALLREDUCE') == '1'

    def update(self, gscale=1.0):
        """[all-reduce of the flat gradient over the group] -> clamp -> adam -> lr decay.  The collective is the
        host's: the library hands out the device pointer of wrapperdW, its main stream, the encoder's flat range and a
        "encoder gradients are final" wait.  Two buckets: the encoder's tensors start reducing on a
        communication stream as soon as the encoder backward has ended -- underneath the option-LSTM backward --
        the shared embedding and the decoder's tensors follow behind the step on the library's main stream."""
        if self.library_comm:
            import os
            from .parallel import library_comm_world
            world = library_comm_world()
            assert world > 0, "library_comm=True but no communicator: call visdial_amd.parallel.init_library_comm first"
            if world > 1 or os.environ.get('VD_FORCE_ALLREDUCE') == '1':
                call("vd_model_allreduce_grads", self.h)        # two buckets, library-owned communication stream
                gscale = 1.0 / world
        elif self._dp_active():
            import torch
            from .parallel import reduce_gradients
            if self._dW is None:
                ptrs = [C.c_void_p() for _ in range(4)]
                call("vd_model_flat_pointers", self.h, *[C.byref(x) for x in ptrs])
                n = int(_lib.load().vd_model_flat_size(self.h))
                self._dW = torch.as_tensor(_DevArray(ptrs[1].value, n), device='cuda')
                self._stream = torch.cuda.ExternalStream(_lib.load().vd_model_stream(self.h))
                self._comm = torch.cuda.Stream()
                lo, hi = C.c_int64(), C.c_int64()
                call("vd_model_encoder_range", self.h, C.byref(lo), C.byref(hi))
                self._enc_range = (int(lo.value), int(hi.value))
            lo, hi = self._enc_range
            work = None
            if hi > lo:
                call("vd_model_wait_encoder_grads", self.h, C.c_void_p(self._comm.cuda_stream))
                with torch.cuda.stream(self._comm):
                    _, work = reduce_gradients(self._dW[lo:hi], self.dist_group, async_op=True)
            with torch.cuda.stream(self._stream):          # ordered behind the step on the library's main stream
                for sl in (self._dW[:lo], self._dW[hi:]):
                    gscale, _ = reduce_gradients(sl, self.dist_group)
                if work is not None:
                    work.wait()                            # the main stream waits for bucket 1
                    self._stream.wait_stream(self._comm)
        call("vd_model_update", self.h, float(gscale))

    def trainIteration(self, dataloader):
        """model.lua:66-106, software-pipelined like Model.trainIteration: enqueue the step, upload the next batch
        (copy stream, second slot) while the device executes, then wait for this step's loss."""
        if self._keep is None or self._keep is not dataloader:
            # nothing usable in the library's slot: first call, another dataloader, or evaluate / retrieve / predict
            # replaced the prefetched batch.  The batch drawn for this step is still on the host: upload it again
            # (the dataloader's sample stream is not advanced twice).
            if self._next_batch is not None and self._next_src is dataloader:
                self.upload(self._next_batch)
            else:
                self.upload(self._train_batch(dataloader))
        numTokens = self._numTokens                             # of the batch this step trains on
        call("vd_model_forward_backward", self.h, 0)
        self.update()
        self._next_batch, self._next_src = self._train_batch(dataloader), dataloader
        self.upload(self._next_batch)                           # prefetch: the second slot, on the copy stream
        self._keep = dataloader                                 # (upload() clears it: set AFTER the prefetch)
        curLoss = self.loss()
        # model.lua:73-93: gen feeds curLoss / numTokens into the EMA (the criterion sums over tokens), disc curLoss
        cur = curLoss / max(numTokens, 1.0) if self.params['decoder'] == 'gen' else curLoss
        self.runningLoss = 0.95 * self.runningLoss + 0.05 * cur if self.runningLoss > 0 else cur
        return curLoss

    def scores(self, N, O):
        a = np.empty((N, O), np.float32)
        call("vd_model_scores", self.h, a.ctypes.data, a.size)
        return a

    def retrieveBatch(self, batch, useGt=None):
        """model.lua:344-430: ground-truth ranks [N] (useGt; default params['useGt']) or all ranks [N x O]"""
        if useGt is None:
            useGt = bool(self.params.get('useGt', True))
        self.upload(batch)
        return self._retrieved_ranks(useGt)

    def _retrieved_ranks(self, useGt):
        """retrieve the batch in the slot through the configured head; the ground-truth ranks [N] (useGt) or all ranks [N x O]"""
        # params fusedLhood: the generative decoder's candidates through the live-row log-likelihood head (a disc model: argument error);
        # a model created with fusedLhood = 2 scores them over the prefix tree behind the same call
        call("vd_model_retrieve_lhood" if int(self.params.get('fusedLhood', 0) or 0) else "vd_model_retrieve", self.h)
        N, O = self._N, int(self.params.get('numOptions', 100))
        out = np.empty(N if useGt else (N, O), np.int32)
        call("vd_model_ranks", self.h, int(useGt), out.ctypes.data)
        return out

    def retrieve_rollout_batch(self, batch):
        """All ranks [N x O] of `batch` on a history the model wrote itself (split_eval.py E1-E5), the history at its untrimmed width.
        decoder disc, a model created with params retrieveRollout = 1: ONE upload and ONE vd_model_retrieve, which runs the R passes on
        the device.  decoder gen, a model created with params beamRollout = 1 and given params rolloutBeam = dict(beamSize, beamLen,
        startToken, endToken): one upload, vd_model_encode, vd_model_beam_search -- which leaves the generated history in the batch's
        slot -- and vd_model_retrieve (params fusedLhood: _lhood) on that slot.  Any other model: the host loop."""
        self._rollout_answers = None
        gen = self.params['decoder'] == 'gen'
        if 'hist' not in batch or not self._knobs['beamRollout' if gen else 'retrieveRollout']:
            return SplitEval.retrieve_rollout_batch(self, batch)
        if self._knobs['rolloutConcatEnd'] != self._concat_end():
            raise ValueError("rollout = 1 with rolloutHistory = %r (<END> = %d), but this model was created with rolloutConcatEnd = %d: the device "
                             "rollout takes its history rule when the model is created (params rolloutConcatEnd of NativeModel)"
                             % (self.params.get('rolloutHistory', 'row'), self._concat_end(), self._knobs['rolloutConcatEnd']))
        self.upload(batch)
        if gen:
            beam = self.params.get('rolloutBeam')
            if not beam:
                raise ValueError("rollout = 1 with decoder 'gen' needs params rolloutBeam = dict(beamSize, beamLen, startToken, endToken)")
            call("vd_model_encode", self.h)
            self._rollout_answers = (self._gen_beam(beam['beamSize'], beam['beamLen'], beam['startToken'], beam['endToken'])[0],
                                     int(beam['endToken']))
        return self._retrieved_ranks(False)

    def rollout_history(self, batch, ranks, cut=None):
        if getattr(self, '_rollout_answers', None) is None:
            return SplitEval.rollout_history(self, batch, ranks, cut)
        tokens, end = self._rollout_answers                       # decoder gen: the beam search's answers (R2 / R3; CH1 - CH4)
        return rollout_answered_history(batch, tokens, end, self._concat_end(), cut)

    # Model:evaluate / retrieve / predict (model.lua:109-246): visdial_amd/split_eval.py, shared with the Python host
    def _set_training(self, on):
        self.training(on)

    # Model:generateAnswers (host loop in split_eval.py); the four device steps through the model-level ABI
    def _gen_encode(self, batch):
        self.upload({k: v for k, v in batch.items() if k in ('ques_fwd', 'hist', 'img_feat', 'img_regions')})
        call("vd_model_encode", self.h)

    def _gen_begin(self, rounds):
        r = np.ascontiguousarray(rounds, dtype=np.int32)
        call("vd_model_decode_begin", self.h, r.ctypes.data, r.size)
        self._gen_n = r.size

    def _gen_step(self, tokens):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        assert t.size == self._gen_n
        out = np.empty((t.size, int(self.params['vocabSize'])), np.float32)
        call("vd_model_decode_step", self.h, t.ctypes.data, out.ctypes.data)
        return out

    def _gen_select(self, src, n_keep):
        s_ = np.ascontiguousarray(src, dtype=np.int32)
        call("vd_model_decode_select", self.h, s_.ctypes.data, int(n_keep))

    def _gen_beam(self, beamSize, beamLen, startToken, endToken):
        """the batched beam search (beamBatch > 0) of every round of the last `_gen_encode` batch: vd_model_beam_search.  Returns (tokens
        [N x beamLen], scores [N]); a model created with params beamGroups = G > 1 returns every group's answer, (tokens
        [N x G x beamLen], scores [N x G])."""
        N, G = int(self._N), self._knobs['beamGroups']
        tokens = np.zeros((N * G, int(beamLen)), np.int32)
        scores = np.zeros(N * G, np.float64)
        call("vd_model_beam_search", self.h, int(beamSize), int(beamLen), int(startToken), int(endToken), tokens.ctypes.data,
             scores.ctypes.data)
        if G > 1:
            return tokens.reshape(N, G, int(beamLen)), scores.reshape(N, G)
        return tokens, scores

    def _created_with(self, batch, taker, noun, asked, compare=None, say=None):
        """the values generateAnswers asks for, {params key: value}, against the ones the model was created with"""
        made = {k: self._knobs[k] for k in asked}
        asked = {k: type(made[k])(v) for k, v in asked.items()}
        if any(asked[k] != made[k] for k in compare or asked):
            show = lambda d, names: ' / '.join(('%s = %d' if isinstance(v, int) else '%s = %g') % (n, v) for n, v in zip(names, d.values()))
            raise ValueError("%s > 0 with %s, but this model was created with %s: the device %s takes its %s when the model is created "
                             "(params %s of NativeModel)" % (batch, show(asked, say or asked), show(made, made), taker, noun, ' / '.join(made)))

    def _beam_grouping(self, groups, diversity):
        self._created_with('beamBatch', 'search', 'groups', dict(beamGroups=groups, beamDiversity=diversity),
                           compare=None if self._knobs['beamGroups'] > 1 else ('beamGroups',))

    def _beam_constraints(self, minLen, noRepeat, lengthPenalty):
        self._created_with('beamBatch', 'search', 'constraints', dict(beamMinLen=minLen, beamNoRepeat=noRepeat, beamLengthPenalty=lengthPenalty))

    def _beam_rollout(self, rollout):
        self._created_with('beamBatch', 'search', 'rollout', dict(beamRollout=rollout), say=('rollout',))

    def _sample_truncation(self, topK, topP):
        self._created_with('sampleBatch', 'sampler', 'truncation', dict(topK=topK, topP=topP))

    def _gen_sample(self, beamLen, startToken, endToken, temperature, uniforms):
        """the batched temperature sampling (sampleBatch > 0) of every round of the last `_gen_encode` batch with the host's
        uniforms [beamLen x N]: vd_model_sample; over the top-k / nucleus kept set if the model was created with params topK / topP.  Returns (tokens [N x (beamLen + 1)], fp64 log-likelihoods [N])."""
        N, L = int(self._N), int(beamLen)
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        if u.shape != (L, N):
            raise ValueError('uniforms must be [beamLen x N] = [%d x %d], got %s' % (L, N, u.shape))
        tokens = np.zeros((N, L + 1), np.int32)
        loglik = np.zeros(N, np.float64)
        call("vd_model_sample", self.h, L, int(startToken), int(endToken), float(temperature), u.ctypes.data, tokens.ctypes.data,
             loglik.ctypes.data)
        return tokens, loglik

    def option_rows(self):
        """(rows the option LSTM executes, N * O candidates) of the current batch: the upload de-duplicates candidates; with
        params optionCache in evaluation mode the rows the cache did not hold (possibly 0); after a training step on a live attachment
        the candidate rows of the live rounds"""
        a, b = C.c_int64(), C.c_int64()
        call("vd_model_option_rows", self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def family_ms(self):
        a = (C.c_float * 3)()
        call("vd_model_family_ms", self.h, a)
        return [float(x) for x in a]

    def synchronize(self):
        call("vd_model_synchronize", self.h)
