"""ctypes binding of libpoccala_hip.so (C-ABI: include/poccala_hip.h).

The HIP library is the product; there is NO CPU fallback.  Importing this module
without the built library, or calling into it without a GPU, raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('POCCALA_HIP_LIB', os.path.join(_HERE, 'libpoccala_hip.so'))   # override: kernel A/B builds

PCL_F32, PCL_F64 = 0, 1
PCL_MODEL_Q1_SUMVAR, PCL_MODEL_LOGDET = 0, 1
PCL_ROW_ENTRY, PCL_ROW_EXIT = -1, -2
PCL_MAX_PASS = 16
PCL_VAD_DIST_IN, PCL_VAD_OSF_IN = 1, 2
PCL_FRONTEND_NO_VAD, PCL_FRONTEND_KEEP_F64 = 1, 2
PCL_PITCH_NCCF_IN = 1
PCL_MLLR_OK, PCL_MLLR_LOW_OCCUPANCY, PCL_MLLR_FEW_MIXTURES, PCL_MLLR_NOT_POSITIVE_DEFINITE = 0, 1, 2, 3
PCL_CMVN_OK, PCL_CMVN_LOW_COUNT, PCL_CMVN_NOT_FINITE = 0, 1, 2
SEG_GET = dict(counts=0, order=1, assign=2, seeds=3)
GET = dict(B=0, alpha=1, beta=2, lgamma=3, ksai=4, gamma=5, pi=6, logp=7, npass=8, qtrace=9, path=10, point=11, ksai_nz=12)

# every symbol include/poccala_hip.h declares: (restype, argtypes)
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
PROTOTYPES = {
    'pcl_init': (_i, [_i, C.POINTER(_vp)]),
    'pcl_destroy': (_i, [_vp]),
    'pcl_last_error': (C.c_char_p, [_vp]),
    'pcl_sync': (_i, [_vp]),
    'pcl_pool_stats': (_i, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    'pcl_device_info': (_i, [_vp, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_size_t)]),
    'pcl_kernel_time': (_i, [_vp, C.c_char_p, C.POINTER(C.c_float), C.POINTER(_i)]),
    'pcl_model_upload': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i]),
    'pcl_frames_upload': (_i, [_vp, C.c_int64, _i, _vp, _i]),
    'pcl_frames_stage': (_i, [_vp, C.c_int64, _i, _vp]),
    'pcl_frames_swap': (_i, [_vp]),
    'pcl_host_alloc': (_i, [_vp, C.c_size_t, C.POINTER(C.c_void_p)]),
    'pcl_host_free': (_i, [_vp, _vp]),
    'pcl_batch_create': (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(_vp)]),
    'pcl_batch_destroy': (_i, [_vp]),
    'pcl_batch_set_transitions': (_i, [_vp, _vp, _vp]),
    'pcl_batch_set_states': (_i, [_vp, _vp]),
    'pcl_batch_set_emissions': (_i, [_vp, _vp]),
    'pcl_batch_set_posteriors': (_i, [_vp, _vp]),
    'pcl_batch_score': (_i, [_vp, _i]),
    'pcl_batch_forward_backward': (_i, [_vp, _i, _d]),
    'pcl_batch_viterbi': (_i, [_vp, _i]),
    'pcl_batch_mbr': (_i, [_vp, _vp, _d, _i]),
    'pcl_batch_mbr_get': (_i, [_vp, _vp, _vp, _vp, _vp]),
    'pcl_batch_mbr_posteriors': (_i, [_vp, _i]),
    'pcl_batch_get': (_i, [_vp, _i, _vp]),
    'pcl_batch_sizes': (_i, [_vp, _vp, _vp, _vp, _vp]),
    'pcl_batch_fetch_async': (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    'pcl_batch_fetch_wait': (_i, [_vp]),
    'pcl_clock_probe': (_i, [_vp, _i, C.POINTER(C.c_double)]),
    'pcl_stats_zero': (_i, [_vp]),
    'pcl_batch_accumulate': (_i, [_vp, _i]),
    'pcl_accumulate_prune': (_i, [_vp, C.c_double]),
    'pcl_stats_download': (_i, [_vp, _vp, _vp, _vp, _vp]),
    'pcl_mstep': (_i, [_vp, _d]),
    'pcl_seg_create': (_i, [_vp, C.c_int64, _i, _vp, C.POINTER(_vp)]),
    'pcl_seg_destroy': (_i, [_vp]),
    'pcl_seg_get': (_i, [_vp, _i, _vp]),
    'pcl_seg_kmeans': (_i, [_vp, _i, C.c_uint64, _i, _i, _vp, _vp]),
    'pcl_seg_centres': (_i, [_vp, _vp]),
    'pcl_seg_em': (_i, [_vp, _d, _d, _i, _i, _vp, _vp, _vp]),
    'pcl_model_download': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_frames_moments': (_i, [_vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    'pcl_model_flat_start': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i]),
    'pcl_flat_start': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    'pcl_uniform_segments': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, C.POINTER(_vp)]),
    'pcl_model_mixup': (_i, [_vp, _i, _d, _vp]),
    'pcl_mllr_estimate': (_i, [_vp, _i, _vp, _d, _vp, _vp, _vp]),
    'pcl_model_transform_means': (_i, [_vp, _i, _vp, _vp]),
    'pcl_mstep_map': (_i, [_vp, _d]),
    'pcl_ebw_hold': (_i, [_vp]),
    'pcl_ebw_drop': (_i, [_vp]),
    'pcl_ebw_stats_download': (_i, [_vp, _vp, _vp, _vp, _vp]),
    'pcl_mstep_ebw': (_i, [_vp, _d, _d, _d, _i, _vp, _vp]),
    'pcl_fmllr_zero': (_i, [_vp, _i]),
    'pcl_batch_accumulate_fmllr': (_i, [_vp, _vp]),
    'pcl_fmllr_stats_download': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_fmllr_estimate': (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp]),
    'pcl_frames_transform': (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp]),
    'pcl_mllt_zero': (_i, [_vp, _vp]),
    'pcl_batch_accumulate_mllt': (_i, [_vp, _vp]),
    'pcl_mllt_stats_download': (_i, [_vp, _vp, _vp]),
    'pcl_mllt_estimate': (_i, [_vp, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcl_lda_zero': (_i, [_vp, _i, _i, _i]),
    'pcl_lda_accumulate': (_i, [_vp, _i, _vp, _vp, _vp]),
    'pcl_batch_accumulate_lda': (_i, [_vp, _vp]),
    'pcl_lda_stats_download': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_frames_splice_project': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    'pcl_frames_download': (_i, [_vp, _vp, _vp]),
    'pcl_cmvn_zero': (_i, [_vp, _i]),
    'pcl_cmvn_accumulate': (_i, [_vp, _i, _vp, _vp, _vp]),
    'pcl_cmvn_stats_download': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_frames_cmvn': (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _d, C.c_int64, _vp]),
    'pcl_frames_cmvn_sliding': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _d]),
    'pcl_tree_zero': (_i, [_vp, _i]),
    'pcl_tree_accumulate': (_i, [_vp, _i, _vp, _vp, _vp]),
    'pcl_batch_accumulate_tree': (_i, [_vp, _vp]),
    'pcl_tree_stats_shape': (_i, [_vp, _vp, _vp]),
    'pcl_tree_stats_download': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_tree_stats_upload': (_i, [_vp, _vp, _vp, _vp]),
    'pcl_tree_build': (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, C.c_int64, _d, _i, _d, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, _vp]),
    'pcl_tying_upload': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i]),
    'pcl_tying_drop': (_i, [_vp]),
    'pcl_tying_lookup': (_i, [_vp, _i, _vp, _vp]),
    'pcl_batch_get_states': (_i, [_vp, _vp, _vp]),
    'pcl_batch_create_labels_tied': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    'pcl_model_conditioning': (_i, [_vp, _vp, _vp]),
    'pcl_model_split_info': (_i, [_vp, _vp, _vp]),
    'pcl_coarse_counter': (_i, [_vp, _vp, _i]),
    'pcl_coarse_counters': (_i, [_vp, _vp, _vp, _i]),
    'pcl_score_occupancy': (_i, [_vp, _i]),
    'pcl_batch_regroup': (_i, [_vp, _vp, _i, _vp, _vp]),
    'pcl_batch_align_segments': (_i, [_vp, _vp, _vp, C.POINTER(_vp)]),
    'pcl_mfcc': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_int64]),
    'pcl_mfcc_pcm16': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_int64]),
    'pcl_vad': (_i, [_vp, _i, _vp, _vp, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp]),
    'pcl_frontend': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, C.c_int64]),
    'pcl_frontend_pcm16': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _d, _i, _vp, _vp, _vp, C.c_int64]),
    'pcl_pitch': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _d, _d, _d, _d, _d, _vp, _i, _i, _vp, _vp, _vp, _vp, C.c_int64]),
    'pcl_pitch_pcm16': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _d, _d, _d, _d, _d, _vp, _i, _i, _vp, _vp, _vp, _vp, C.c_int64]),
    'pcl_frontend_pitch': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _d, _i, _d, _d, _d, _d, _d, _vp, _i,
                                _vp, _vp, _vp, C.c_int64]),
    'pcl_frontend_pitch_pcm16': (_i, [_vp, _i, _vp, _vp, _i, _d, _d, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _d, _i, _d, _d, _d, _d, _d, _vp, _i,
                                      _vp, _vp, _vp, C.c_int64]),
    'pcl_timing_enable': (_i, [_vp, _i]),
    'pcl_device_count': (_i, [C.POINTER(_i)]),
    'pcl_units_upload': (_i, [_vp, _i, _i, _vp, _vp]),
    'pcl_units_download': (_i, [_vp, _vp]),
    'pcl_batch_create_labels': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    'pcl_batch_refresh_transitions': (_i, [_vp]),
    'pcl_batch_accumulate_hmm': (_i, [_vp]),
    'pcl_hmm_acc_zero': (_i, [_vp]),
    'pcl_hmm_acc_download': (_i, [_vp, _vp, _vp]),
    'pcl_mstep_transitions': (_i, [_vp]),
    'pcl_lexicon_upload': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'pcl_batch_decode': (_i, [_vp, _d, _i, _i, _i, _d, _d]),
    'pcl_batch_decode_get': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcl_lm_upload': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcl_batch_decode_lm': (_i, [_vp, _d, _i, _i, _i, _d, _d]),
    'pcl_batch_decode_get_words': (_i, [_vp, _vp]),
    'pcl_lexicon_tie': (_i, [_vp, _vp]),
    'pcl_lexicon_untie': (_i, [_vp]),
    'pcl_lexicon_states': (_i, [_vp, _vp]),
    'pcl_batch_decode_tied': (_i, [_vp, _d, _i, _i, _i, _d, _d, _i]),
    'pcl_batch_decode_lattice': (_i, [_vp, _d, _i, _i, _i, _d, _d, _i, _i, _i]),
    'pcl_batch_lattice_get': (_i, [_vp] * 15),
    'pcl_batch_lattice_posteriors': (_i, [_vp, _d]),
    'pcl_batch_lattice_results': (_i, [_vp] * 8),
    'pcl_batch_lattice_set_records': (_i, [_vp, _i, _i, _i] + [_vp] * 15),
    'pcl_comm_init_host': (_i, [_vp, _i, _i, _vp, _vp]),
    'pcl_comm_info': (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'pcl_em_exchange': (_i, [_vp, _d, _i, _i]),
    'pcl_pipe_info': (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    'pcl_batch_accumulate_exchange': (_i, [_vp, _i, _d, _i, _i, _i]),
    'pcl_accumulate_exchange_idle': (_i, [_vp, _d, _i, _i, _i]),
    'pcl_comm_unique_id': (_i, [_vp]),
    'pcl_comm_init': (_i, [_vp, _i, _i, _vp]),
    'pcl_stats_allreduce': (_i, [_vp]),
    'pcl_comm_destroy': (_i, [_vp]),
}


class PoccalaHipError(RuntimeError):
    """A C-ABI call returned a negative pcl_status."""

    def __init__(self, code, msg):
        super().__init__('libpoccala_hip: %s (status %d)' % (msg, code))
        self.code = code


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)   # pcl_allgather_fn

_lib = None


HW_QUEUES = None      # set by load(): {'value': GPU_MAX_HW_QUEUES as this process has it, 'effective': False if HIP was already loaded}


def _hip_runtime_loaded():
    """True when libamdhip64 is already mapped into this process (its environment knobs were read then)."""
    try:
        with open('/proc/self/maps') as f:
            return any('libamdhip64' in line for line in f)
    except OSError:
        return False


def load():
    """dlopen the library and bind every prototype.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                          '(or make -C poccala_amd/csrc).  There is no CPU fallback.' % LIB_PATH)
    # A context owns five HIP streams (main, dynamic programming, producer / frame staging, descriptors, downloads; the first int16
    # front-end call adds one for its PCM chunks, busy only inside that call while the main stream waits for it).  The runtime
    # multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by default: two of the five then share a queue, and a command
    # that waits for an event (the download of step k waits for its forward-backward) holds up whatever sits behind it in that
    # queue (the scoring kernel of step k + 1).  Read when the HIP runtime starts: set before the library (and with it
    # libamdhip64) is loaded, unless the caller has chosen a value.
    global HW_QUEUES
    hip_was_loaded = _hip_runtime_loaded()
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    HW_QUEUES = dict(value=os.environ['GPU_MAX_HW_QUEUES'], effective=not hip_was_loaded)
    if hip_was_loaded and int(HW_QUEUES['value'] or 0) >= 8:
        # (the variable is read when the HIP runtime starts: a process that imported another HIP user first -- torch -- may run the
        #  five streams of a context on four hardware queues; same results, the step-to-step overlap of bench.py suffers)
        import warnings
        warnings.warn('poccala_amd: libamdhip64 was loaded before this library; GPU_MAX_HW_QUEUES=%s may not be in effect '
                      '(export it before the process starts)' % HW_QUEUES['value'], RuntimeWarning, stacklevel=2)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)        # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a):
    """Pointer to a C-contiguous NumPy array (or None)."""
    if a is None:
        return None
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(C.c_void_p)


def as_c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def all_int16(signals):
    """The front-end's route: True when `signals` is a non-empty sequence of np.int16 arrays and nothing else -- they travel as int16
    (pcl_mfcc_pcm16 / pcl_frontend_pcm16).  Everything else (float arrays, whatever their values; other integer widths; lists; a mixed
    sequence; no signal at all) takes the float64 entry points, as before there was a choice."""
    signals = list(signals) if not isinstance(signals, (list, tuple)) else signals
    return len(signals) > 0 and all(isinstance(s, np.ndarray) and s.dtype == np.int16 for s in signals)


def pack_signals(signals, none_ok=False):
    """What every front-end entry point is handed: (sigs, flat, off, pcm16) -- the signals as 1-D arrays of the wire type (np.int16 when
    all_int16(signals), else np.float64), their concatenation, sig_off (U + 1,) int64, and the route.  No signal at all is a ValueError
    before any call into the library, unless none_ok (pitch_batch, which lets the library refuse it): then `flat` is empty."""
    signals = list(signals)
    pcm16 = all_int16(signals)
    wire = np.int16 if pcm16 else np.float64
    sigs = [np.asarray(s, dtype=wire).reshape(-1) for s in signals]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    if none_ok and not sigs:
        return sigs, np.zeros(0, dtype=wire), off, pcm16
    return sigs, as_c(np.concatenate(sigs), wire), off, pcm16
