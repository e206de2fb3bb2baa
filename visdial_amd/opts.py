"""Command-line options: same flag names and defaults as the reference's opts.lua:5-40, plus the
derived capability flags it infers from the encoder NAME (opts.lua:54-67)."""
import argparse
import ctypes
import math
import time

# (flag, default, help) -- opts.lua:5-40
OPTIONS = [
    ('inputImg', 'data/data_img.h5', 'HDF5 file with image features'),
    ('inputQues', 'data/visdial_data.h5', 'HDF5 file with preprocessed questions'),
    ('inputJson', 'data/visdial_params.json', 'JSON file with info and vocab'),
    ('savePath', 'checkpoints/', 'Path to save checkpoints'),
    ('saveIter', 2, 'Save model checkpoint after every saveIter epochs'),
    ('encoder', 'lf-ques-hist', 'Name of the encoder to use'),
    ('decoder', 'gen', 'Name of the decoder to use (gen/disc)'),
    ('imgNorm', 1, 'normalize the image feature. 1=yes, 0=no'),
    ('imgEmbedSize', 300, 'Size of the multimodal embedding'),
    ('imgFeatureSize', 4096, 'Channel size of the image feature'),
    ('imgSpatialSize', 14, 'Spatial size of image features (for attention-based encoders)'),
    ('embedSize', 300, 'Size of input word embeddings'),
    ('rnnHiddenSize', 512, 'Size of the LSTM state'),
    ('maxHistoryLen', 60, 'Maximum history to consider when using concatenated QA pairs'),
    ('numLayers', 2, 'Number of layers in LSTM'),
    ('commonEmbeddingSize', 512, 'Common embedding size in MN-ATT-QIH'),
    ('numAttentionLayers', 1, 'No. of attention hops in MN-ATT-QIH'),
    ('loadPath', '', 'Checkpoint path to load from'),
    ('batchSize', 40, 'Batch size (number of threads)'),
    ('learningRate', 1e-3, 'Learning rate'),
    ('weightInit', 'xavier', 'Weight initialization strategy (accepted and ignored, as in the reference)'),
    ('dropout', 0.5, 'Dropout'),
    ('numEpochs', 100, 'Epochs'),
    ('LRateDecay', 10, 'unused (as in the reference)'),
    ('lrDecayRate', 0.9997592083, 'Decay for learning rate'),
    ('minLRate', 5e-5, 'Minimum learning rate'),
    ('gpuid', 0, 'GPU id to use'),
    ('backend', 'cudnn', 'accepted for CLI compatibility; ignored'),
    # not a reference flag: the arithmetic of the option recurrence.  DEFAULT = split9 (fp32-grade: every fp32 operand as the exact sum of three
    # bf16 values, all nine products, fp32 accumulate -- what bench.py's headline measures; it applies at throughput shapes, >= 2 048 option rows,
    # smaller recurrences run the fp32 MFMA either way)
    ('lstmPrecision', 'split9', "arithmetic of the option-LSTM recurrence GEMMs: 'split9' (default: exact 3-way bf16 split of both operands, 9 bf16 MFMAs per fp32 one, fp32-grade; applies to the step kernels from 2048 rows, the dWh contraction from 8192 rows and, through the native host, the image attention's dense products from 128 rows (N x S^2); smaller shapes run v_mfma_f32) | 'fp32' (v_mfma_f32_32x32x2_f32) | 'bf16' (BASELINE configs[4]: bf16 operands, fp32 accumulation; through the native host also the encoder's recurrent products and dense weight gradients) | 'split6' / 'split3' (fewer products: data only)"),
    ('saveFormat', 't7', "checkpoint files: 't7' = model_epoch_%d.t7 / model_final.t7 in the Torch7 binary format "
                         "(train.lua:99-102,120-121) | 'pt' = torch.save of the same three fields"),
    ('host', 'python', "which host drives the library: 'python' (operator-level C ABI, visdial_amd/model.py) | 'native' "
                       "(model-level C ABI, the calls lua/model.lua makes; visdial_amd/native.py)"),
]


def derive(opt):
    """opts.lua:54-67: capabilities come from substrings of the encoder file name."""
    enc = opt['encoder']
    opt['useHistory'] = 'hist' in enc
    opt['useIm'] = 'im' in enc
    opt['concatHistory'] = 'lf' in enc
    if 'att' in enc:
        if opt.get('inputImg') == 'data/data_img.h5':
            opt['inputImg'] = 'data/data_img_pool5.h5'
        opt['imgNorm'] = 0
    return opt


def check_dense(opt):
    """what -denseAnnotations cannot be combined with, refused by name before any model exists (the library refuses the same: loss.hip DT5)"""
    if not opt.get('denseAnnotations'):
        return
    if opt.get('decoder') != 'disc':
        raise ValueError("-denseAnnotations with -decoder %s: the dense target trains the option scores of decoder 'disc'" % opt.get('decoder'))
    if float(opt.get('labelSmoothing') or 0.0) > 0.0:
        raise ValueError("-denseAnnotations with -labelSmoothing %r: a dense target is not smoothed; train with -labelSmoothing 0"
                         % (opt.get('labelSmoothing'),))
    mix = float(opt.get('denseMix') or 0.0)
    if not 0.0 <= mix <= 1.0:
        raise ValueError("-denseMix %r must be a finite real in [0, 1] (0 = rounds without an annotation do not train)" % (opt.get('denseMix'),))


def check_dense_rows(opt):
    """what -denseRows live cannot be combined with, refused by name before any model exists (the library refuses the bf16 model: loss.hip DL5)"""
    rows = opt.get('denseRows') or 'all'
    if rows not in ('all', 'live'):
        raise ValueError("-denseRows %r must be 'all' or 'live'" % (rows,))
    if rows != 'live':
        return
    if not opt.get('denseAnnotations'):
        raise ValueError("-denseRows live without -denseAnnotations: the live rounds are those of a dense batch; give the annotation file or "
                         "train with -denseRows all")
    if opt.get('lstmPrecision') == 'bf16':
        raise ValueError("-denseRows live with -lstmPrecision bf16: the compact-state bf16 option recurrence does not run the live rounds' "
                         "rows alone; train with -denseRows all or another -lstmPrecision")


ATT_ENCODERS = ('mn-att-ques-im-hist', 'lf-att-ques-im-hist')    # the encoders with the image attention


def check_img_regions(opt):
    """what -imgRegions M cannot be combined with, refused by name before any model exists (the library refuses the attachment on an encoder
    without the image attention: csrc/attention.hip IR1 - IR6).  -> M"""
    M = opt.get('imgRegions') or 0
    if int(M) != M or M < 0:
        raise ValueError("-imgRegions %r must be an integer >= 0 (0 = off: one S x S grid per image)" % (M,))
    M = int(M)
    if M == 0:
        return 0
    if opt.get('encoder') not in ATT_ENCODERS:
        raise ValueError("-imgRegions %d with -encoder %s: a region count per image masks the image attention, which only %s have"
                         % (M, opt.get('encoder'), ' and '.join(ATT_ENCODERS)))
    if (opt.get('host') or 'python') != 'native':
        raise ValueError("-imgRegions %d: the masked image attention runs in the model-level runtime only: use -host native "
                         "(visdial_amd.native.NativeModel); the operator-level host takes -imgRegions 0" % M)
    return M


def apply_img_regions(opt):
    """-imgRegions M > 0: the padded grid holds S2 = ceil(sqrt(M))^2 >= M rows per image (imgNorm stays 0, as derive sets it for these encoders)"""
    M = check_img_regions(opt)
    if M > 0:
        S = int(math.ceil(math.sqrt(M)))
        while S * S < M:      # (sqrt of a perfect square rounds either way)
            S += 1
        while (S - 1) * (S - 1) >= M:
            S -= 1
        opt['imgSpatialSize'] = S
        print('-imgRegions %d: imgSpatialSize = %d (%d region rows per image, the rows behind an image\'s count are hidden)' % (M, S, S * S))
    return opt


def default_params(**overrides):
    opt = {k: v for k, v, _ in OPTIONS}
    # sizes the reference copies from the dataloader (train.lua:55-59)
    opt.update(vocabSize=11322, maxQuesCount=10, maxQuesLen=20, maxAnsLen=20, numOptions=100)
    opt.update(overrides)
    return derive(opt)


def parse(argv=None):
    ap = argparse.ArgumentParser(description='Train the Visual Dialog model')
    for k, v, h in OPTIONS:
        ap.add_argument('-' + k, '--' + k, type=type(v), default=v, help=h)
    # synthetic-data knobs (no HDF5 offline)
    ap.add_argument('--vocabSize', type=int, default=11322)
    ap.add_argument('--numTrainThreads', type=int, default=2000)
    ap.add_argument('--maxIters', type=int, default=0, help='stop after this many iterations (0 = numEpochs)')
    ap.add_argument('-paramOrder', '--paramOrder', default='',
                    help="flat-vector layout of a .t7 given to -loadPath: '' (this repo's table of the reference's getParameters() order), "
                         "'declaration', or a JSON file: {\"order\": [names]} or the output of lua/dump_param_order.lua under Torch7")
    ap.add_argument('-synthetic', '--synthetic', type=int, default=0,
                    help='1 = allow resuming (-loadPath) on synthetic batches when no dataset files exist')
    # training knobs the reference does not have (-host native; csrc/loss.hip LS1-LS4, csrc/elementwise.hip GC1-GC3, WD1); 0 = off
    ap.add_argument('-labelSmoothing', '--labelSmoothing', type=float, default=0.0,
                    help='(training only, -host native) label smoothing eps in [0, 1): a training target is (1 - eps) onehot + eps / K over the K options (disc) or '
                         'vocabulary words (gen)')
    ap.add_argument('-gradClipNorm', '--gradClipNorm', type=float, default=0.0,
                    help='(training only, -host native) clip the whole gradient to this L2 norm in front of the element clamp at +-5 (a finite real >= 0)')
    ap.add_argument('-weightDecay', '--weightDecay', type=float, default=0.0,
                    help='(training only, -host native) decoupled weight decay lambda: w -= lr * lambda * w beside the Adam step (a finite real >= 0)')
    # dense-annotation fine-tuning (-host native, decoder disc; csrc/loss.hip DT1-DT5)
    ap.add_argument('-denseAnnotations', '--denseAnnotations', default='',
                    help='(training only, -host native, decoder disc) a file of dense relevance annotations of train dialogs: train on batches of '
                         'annotated dialogs with the normalised relevance as the target of the annotated round')
    ap.add_argument('-denseMix', '--denseMix', type=float, default=0.0,
                    help='(with -denseAnnotations) weight mu in [0, 1] of the rounds without an annotation, which keep their one-hot target '
                         '(0 = they do not train)')
    # not a reference flag (kept out of OPTIONS): which candidate rows a dense step executes (csrc/loss.hip DL1-DL5)
    ap.add_argument('-denseRows', '--denseRows', choices=('all', 'live'), default='all',
                    help="(with -denseAnnotations, -host native) 'all' (default): every round's candidates go through the option recurrence and "
                         "its gradients | 'live': only the candidates of the rounds that carry a gradient (weight > 0); the same loss and "
                         "gradients up to fp32 summation order")
    # not a reference flag (kept out of OPTIONS): detector regions, a different number per image (csrc/attention.hip IR1 - IR6)
    ap.add_argument('-imgRegions', '--imgRegions', type=int, default=0,
                    help="(-host native, the two att encoders) M > 0: -inputImg holds regions_<split> [n x M x C] and num_regions_<split> [n]; "
                         "every image attends its own first num_regions rows only.  imgSpatialSize becomes ceil(sqrt(M)).  0 (default) = off")
    opt = vars(ap.parse_args(argv))
    # refused by name before any model exists (the library refuses the same values: csrc/rt_switches.h)
    # (eps is applied in fp32, as in the library: a value that rounds to 1.0f is not below 1)
    if not 0.0 <= ctypes.c_float(opt['labelSmoothing']).value < 1.0:
        ap.error('-labelSmoothing %r must be a real in [0, 1) (0 = off)' % (opt['labelSmoothing'],))
    for k in ('gradClipNorm', 'weightDecay'):
        if not 0.0 <= opt[k] < float('inf'):
            ap.error('-%s %r must be a finite real >= 0 (0 = off)' % (k, opt[k]))
    if not 0.0 <= opt['denseMix'] <= 1.0:
        ap.error('-denseMix %r must be a finite real in [0, 1] (0 = rounds without an annotation do not train)' % (opt['denseMix'],))
    try:
        check_dense(dict(opt, decoder='disc') if opt['loadPath'] else opt)   # (-loadPath: the decoder is the checkpoint's; train.py checks again)
        check_dense_rows(opt)
        if opt['imgRegions'] < 0 or not opt['loadPath']:                     # (-loadPath: the encoder is the checkpoint's; the scripts check again)
            check_img_regions(opt)
    except ValueError as e:
        ap.error(str(e))
    opt.update(maxQuesCount=10, maxQuesLen=20, maxAnsLen=20, numOptions=100)
    if opt['savePath'] == 'checkpoints/':
        t = time.localtime()
        opt['savePath'] = 'checkpoints/model-%d-%d-%d-%d:%d:%d-%s-%s/' % (
            t.tm_mon, t.tm_mday, t.tm_year, t.tm_hour, t.tm_min, t.tm_sec, opt['encoder'], opt['decoder'])
    opt = derive(opt)
    return opt if opt['loadPath'] else apply_img_regions(opt)
