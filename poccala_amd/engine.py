"""Batched host API over the C-ABI (include/poccala_hip.h).

`Engine` owns one GPU context (model + frame matrix + E-step statistics); `Batch` is a set of
sentence-level HMMs processed together.  The drop-in classes in StatisticalModel/ and
AcousticModel/ call these with batch size 1; bench.py and the batched entry points
(`score_labels`, `estep_labels`, `align_labels`) call them with whole corpus shards.

Reference call stacks replaced:
  (B) AcousticModel.multi_embedded_training_1  AcousticModel/AcousticModel.py:884-916
  (C) AcousticModel.multi_process_data         AcousticModel/AcousticModel.py:723-768
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import GET, SEG_GET, PCL_F32, PCL_F64, PCL_MAX_PASS, PCL_ROW_ENTRY, PCL_ROW_EXIT, PoccalaHipError, as_c, ptr


def device_count():
    """HIP devices visible to this process (0 without a GPU)."""
    n = C.c_int(0)
    _lib.load().pcl_device_count(C.byref(n))
    return n.value


class Engine(object):
    """One GPU: `Engine(device)`.  Raises if libpoccala_hip.so is missing or no GPU is present."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        self._ctx = C.c_void_p()
        rc = self._lib.pcl_init(int(device), C.byref(self._ctx))
        if rc != 0:
            msg = self._lib.pcl_last_error(None)
            self._ctx = None
            raise PoccalaHipError(rc, (msg or b'pcl_init failed').decode())
        self.device = int(device)
        self.J = self.M = self.D = 0
        self.n_units = self.S = 0
        self.F = self.FD = 0
        self._model_key = self._frames_key = None
        self._stream_pool, self._stream_pinned = {}, [None]       # Decoder.decode_stream: batches per chunk shape, staging buffer
        self._segments = weakref.WeakSet()  # live Segments objects: closed with the engine
        self._batches = weakref.WeakSet()   # live batches: destroyed before the context (a sweep makes millions: dead ones leave by themselves)
        self._pinned = []    # page-locked host allocations (pinned_empty)
        self._pinned_sizes, self._pinned_named = {}, {}
        self._slot_busy = {}   # result slot -> weakref of the batch with un-waited copies into it
        self._staged = None

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise PoccalaHipError(rc, self._lib.pcl_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, '_ctx', None):
            for b in list(self._batches):
                b.close()
            for sg in list(self._segments):
                sg.close()
            self._batches = weakref.WeakSet()
            self._stream_pool, self._stream_pinned = {}, [None]
            self._lib.pcl_sync(self._ctx)             # result copies into the page-locked buffers freed below may still be in flight
            for p in self._pinned:
                self._lib.pcl_host_free(self._ctx, p)
            self._pinned, self._pinned_sizes, self._pinned_named = [], {}, {}
            self._lib.pcl_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self._lib.pcl_sync(self._ctx))

    @staticmethod
    def pool_stats():
        """The process-wide device memory pool's books (pcl_pool_stats): blocks / bytes handed out and not yet given back, bytes cached,
        hipMalloc calls and device-wide waits so far."""
        blocks, nbytes, cached = C.c_size_t(), C.c_size_t(), C.c_size_t()
        allocs, waits = C.c_uint64(), C.c_uint64()
        _lib.load().pcl_pool_stats(C.byref(blocks), C.byref(nbytes), C.byref(cached), C.byref(allocs), C.byref(waits))
        return dict(handed_out_blocks=blocks.value, handed_out_bytes=nbytes.value, cached_bytes=cached.value,
                    device_allocs=allocs.value, device_waits=waits.value)

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int()
        mem = C.c_size_t()
        self._check(self._lib.pcl_device_info(self._ctx, name, 256, C.byref(cus), C.byref(mem)))
        return dict(name=name.value.decode(), cus=cus.value, hbm_bytes=mem.value)

    def enable_timing(self, on=True):
        """Record HIP events around every kernel launch for `kernel_time` (off by default: a training run pays nothing)."""
        self._check(self._lib.pcl_timing_enable(self._ctx, 1 if on else 0))

    def kernel_time(self, which):
        """(total_ms, launches) of a kernel group since the last query (HIP events on the ctx stream; `enable_timing` first)."""
        ms = C.c_float()
        n = C.c_int()
        self._check(self._lib.pcl_kernel_time(self._ctx, which.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def clock_probe(self, spin_us=1000):
        """The shader clock (MHz) the chip holds right now, measured on the device beside whatever is running (s_memtime against
        the constant 100 MHz s_memrealtime over `spin_us` microseconds); rocm-smi's sclk is the requested level."""
        mhz = C.c_double()
        self._check(self._lib.pcl_clock_probe(self._ctx, int(spin_us), C.byref(mhz)))
        return mhz.value

    # ------------------------------------------------------------------ model / frames
    def load_model(self, mean, var, weight, logdet=False):
        """mean, var (J,M,D) -- var is the DIAGONAL of the reference's (M,D,D) covariance (util.py:23);
        weight (J,M).  `logdet=True` swaps quirk Q1's constant for the textbook one (not parity)."""
        mean = as_c(mean, np.float64)
        var = as_c(var, np.float64)
        weight = as_c(weight, np.float64)
        if mean.ndim != 3 or var.shape != mean.shape or weight.shape != mean.shape[:2]:
            raise ValueError('model shapes: mean %s var %s weight %s' % (mean.shape, var.shape, weight.shape))
        J, M, D = mean.shape
        key = self._digest((mean, var, weight), ('model', bool(logdet)))
        if key is not None and key == self._model_key:
            return                                   # the same content is resident (and no M-step has touched it)
        self._check(self._lib.pcl_model_upload(self._ctx, J, M, D, ptr(mean), ptr(var), ptr(weight),
                                               1 if logdet else 0))
        self.J, self.M, self.D = J, M, D
        self._model_key = key

    _DIGEST_MAX = 64 << 20

    @staticmethod
    def _digest(arrays, tag):
        """Content key of small uploads (the drop-in classes re-send the same unit model / utterance for every call);
        None above 64 MB, where hashing would cost more than it saves."""
        if sum(a.nbytes for a in arrays) > Engine._DIGEST_MAX:
            return None
        head = repr((tag, [(a.shape, str(a.dtype)) for a in arrays])).encode()
        try:                                   # a 128-bit non-cryptographic hash at memory speed where it is installed
            import xxhash
            h = xxhash.xxh3_128(head)
        except ImportError:
            import hashlib
            h = hashlib.blake2b(head, digest_size=16)
        for a in arrays:
            h.update(memoryview(np.ascontiguousarray(a)).cast('B'))
        return h.digest()

    def load_frames(self, frames):
        """(F,D) float32 or float64 MFCC rows of every utterance of the shard, concatenated."""
        frames = np.asarray(frames)
        if frames.ndim != 2:
            raise ValueError('frames must be (F,D)')
        if frames.dtype == np.float32:
            f, dt = as_c(frames, np.float32), PCL_F32
        else:
            f, dt = as_c(frames, np.float64), PCL_F64
        key = self._digest((f,), 'frames')
        if key is not None and key == self._frames_key:
            return
        self._check(self._lib.pcl_frames_upload(self._ctx, f.shape[0], f.shape[1], ptr(f), dt))
        self.F, self.FD = f.shape[0], f.shape[1]
        self._frames_key = key

    def frontend(self, signals, framerate, vec_num=13, sampletime=0.025, overlap=0.5, nfft=512, filterbanks=26, cal_energy=True,
                 d1=True, d2=True, vad=True, simple_size=16, alpha=0.5, beta=0.93, keep_f64=False, fetch=False, pitch=False, f_min=50.,
                 f_max=400., ballast=7000., soft_min_f0=10., pf=0.1):
        """PCM -> resident frames: MFCC (AudioProcessing.MFCC.mfcc), the voice-activity detector (AudioProcessing.VAD.mfcc) and the
        compaction of its survivors in one call, without the features leaving the device -- AcousticModel.__load_audio
        (AcousticModel.py:463-477) for a list of signals.  Afterwards the survivors are the current frame matrix, exactly as
        load_frames(np.float32(rows)) would have left them; returns (lens (U,) int32, begin (U,) int64) for label_batch / batch /
        all_state_batch -- an utterance that kept no frame has length 0 and must be left out of the lists handed to them (lens > 0:
        a batch takes utterances of at least one frame; AcousticModel's batch helpers, which take host arrays, skip empty ones
        themselves).  If no frame of any utterance survives, every length is 0 and the frame matrix is empty.  vad=False: every MFCC row is kept.  keep_f64: the float64 copy parity mode reads is kept too instead of being derived
        from the float32 rows.  fetch=True: (lens, begin, rows) with rows the (sum lens, D) float64 survivors, for inspection.
        When EVERY signal is an np.int16 array (what a wav file holds, and what AudioProcessing.MFCC.init_audio reads) the samples are
        concatenated and sent as int16 (pcl_frontend_pcm16: a quarter of the bytes, page-locked staging, no float64 copy on the host)
        and become float64 in the kernel -- the same bits as the float64 route, which anything else takes (float arrays that hold
        integers, mixed lists, Python lists): nothing is rounded silently.
        pitch=True (pcl_frontend_pitch): three more columns behind the MFCC's -- voicing, ln f0, delta ln f0 over f_min .. f_max Hz
        (AudioProcessing.pitch_batch's, rule P1-P5) -- so the rows are vec_num * {1,2,3} + 3 wide.  The detector still sees the MFCC columns
        alone: lens, begin and the MFCC columns are those of pitch=False bit for bit.  The default takes the call it always took."""
        from .StatisticalModel.AudioProcessing import frame_count, mfcc_dim, mfcc_flags, mfcc_tables, pitch_lags
        sigs, flat, off, pcm16 = _lib.pack_signals(signals)
        rows = int(sum(frame_count(len(s), framerate, sampletime, overlap) for s in sigs))
        mflags = mfcc_flags(cal_energy, d1, d2)
        dim = mfcc_dim(vec_num, mflags) + (3 if pitch else 0)
        tables = mfcc_tables(framerate, vec_num, nfft, filterbanks)
        flags = (0 if vad else _lib.PCL_FRONTEND_NO_VAD) | (_lib.PCL_FRONTEND_KEEP_F64 if keep_f64 else 0)
        lens, begin = np.empty(len(sigs), dtype=np.int32), np.empty(len(sigs), dtype=np.int64)
        out = np.empty((max(rows, 1), dim)) if fetch else None
        # the four entry points take the same arguments, the pitch ones theirs between the detector's and the outputs
        args = [self._ctx, len(sigs), ptr(flat), ptr(off), int(framerate), float(sampletime), float(overlap), int(nfft), int(filterbanks),
                int(vec_num), mflags] + [ptr(t) for t in tables] + [int(simple_size), float(alpha), float(beta), flags]
        if pitch:
            g = pitch_lags(framerate, f_min, f_max)[2]
            args += [float(f_min), float(f_max), float(ballast), float(soft_min_f0), float(pf), ptr(g), int(len(g))]
        call = getattr(self._lib, 'pcl_frontend' + ('_pitch' if pitch else '') + ('_pcm16' if pcm16 else ''))
        self._check(call(*args, ptr(lens), ptr(begin), ptr(out), C.c_int64(rows)))
        self.F, self.FD = int(lens.sum()), dim
        self._frames_key = None
        return (lens, begin, out[:self.F].copy()) if fetch else (lens, begin)

    # ------------------------------------------------------------------ streaming (BASELINE config 5: a corpus fed chunk by chunk)
    def stage_frames(self, frames):
        """Queue the H2D copy of the NEXT chunk's (F,D) float32 rows on the copy stream, into the frame slot that is not
        current; returns at once.  The array must stay untouched until swap_frames() returns (a pinned_empty() array makes
        the copy truly asynchronous)."""
        f = np.asarray(frames)
        if f.ndim != 2 or f.dtype != np.float32 or not f.flags['C_CONTIGUOUS']:
            raise ValueError('stage_frames: a C-contiguous (F,D) float32 array')
        self._check(self._lib.pcl_frames_stage(self._ctx, f.shape[0], f.shape[1], ptr(f)))
        self._staged = f

    def swap_frames(self):
        """Wait for the staged copy and make that chunk the current frame matrix (batches created from now on index it)."""
        self._check(self._lib.pcl_frames_swap(self._ctx))
        self.F, self.FD = self._staged.shape
        self._staged = None
        self._frames_key = None

    def pinned_empty(self, shape, dtype=np.float32):
        """A NumPy array over page-locked host memory (freed with the engine)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._lib.pcl_host_alloc(self._ctx, n, C.byref(p)))
        self._pinned.append(p)
        self._pinned_sizes[p.value] = n
        buf = (C.c_char * n).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def pinned_free(self, arr_or_ptr):
        """Release one pinned_empty() allocation before the engine closes."""
        addr = arr_or_ptr if isinstance(arr_or_ptr, int) else arr_or_ptr.__array_interface__['data'][0]
        for k, p in enumerate(self._pinned):
            if p.value == addr:
                self._lib.pcl_host_free(self._ctx, p)
                del self._pinned[k]
                self._pinned_sizes.pop(addr, None)
                for name in [n for n, a in self._pinned_named.items() if a.__array_interface__['data'][0] == addr]:
                    del self._pinned_named[name]
                return
        raise ValueError('not a pinned_empty() allocation of this engine')

    def pinned_bytes(self):
        """Page-locked host bytes this engine holds (soak tests assert that a ragged stream keeps it bounded)."""
        return int(sum(self._pinned_sizes.get(p.value, 0) for p in self._pinned))

    def _pinned_views(self, name, shapes):
        """Arrays of the given (shape, dtype) list over ONE grow-only page-locked buffer per name (kept with the engine, reused by
        every caller of that name; grown by doubling).  A block that was outgrown is RETIRED, not freed: views handed out earlier
        may still be alive (a dict from an earlier result_buffers() call passes fetch_async's size checks), and an asynchronous
        DMA into freed page-locked memory corrupts the host.  Retired blocks go with the engine; doubling bounds
        them by the size of the live block."""
        need = [int(np.prod(sh)) * np.dtype(dt).itemsize for sh, dt in shapes]
        off = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in need])])
        total = int(off[-1]) or 64
        cur = self._pinned_named.get(name)
        if cur is None or cur.nbytes < total:
            cur = self.pinned_empty((max(total, 2 * (cur.nbytes if cur is not None else 0)),), np.uint8)
            self._pinned_named[name] = cur               # (the outgrown block stays in self._pinned until close())
        return [cur[int(off[k]):int(off[k]) + need[k]].view(dt).reshape(sh) for k, (sh, dt) in enumerate(shapes)]

    def _slots_of(self, arrays):
        """result slots whose LIVE block holds any of the arrays"""
        out = set()
        for a in arrays:
            addr = a.__array_interface__['data'][0]
            for name, blk in self._pinned_named.items():
                if name.startswith('fetch_results_'):
                    lo = blk.__array_interface__['data'][0]
                    if lo <= addr < lo + blk.nbytes:
                        out.add(int(name[len('fetch_results_'):]))
        return out

    def batch(self, N, T, frame_begin=None):
        return Batch(self, N, T, frame_begin)

    def segments(self, frame_state, J=None):
        """Per-state frame lists of the loaded frame matrix for segmental training (training scheme 1): frame_state[t] = the GMM
        state that owns frame t, or -1 (unused).  J defaults to the loaded model's."""
        return Segments(self, frame_state, self.J if J is None else J)

    # ------------------------------------------------------------------ starting from nothing: flat start, uniform segmentation
    def _utt_ranges(self, T, frame_begin):
        T = as_c(T, np.int32).reshape(-1)
        fb = None if frame_begin is None else as_c(frame_begin, np.int64).reshape(-1)
        if T.size == 0 or (fb is not None and fb.shape != T.shape):
            raise ValueError('T and frame_begin must be equal-length, non-empty')
        return T, fb

    def frames_moments(self, T, frame_begin=None, n_utts=None, step=1):
        """Global mean and variance of data[::step] of the first n_utts utterances of the resident frames (default: all), as
        AcousticModel.__flat_start takes them (AcousticModel.py:492-501): (mean (D,), var (D,), n_rows).  The variance is about that
        mean, divided by n, floored at 1e-4.  frame_begin=None: the utterances lie back to back from row 0."""
        T, fb = self._utt_ranges(T, frame_begin)
        mean, var = np.empty(max(self.FD, 1)), np.empty(max(self.FD, 1))
        n = np.zeros(1, dtype=np.int64)
        self._check(self._lib.pcl_frames_moments(self._ctx, T.size, ptr(T), ptr(fb), int(T.size if n_utts is None else n_utts), int(step),
                                                 ptr(mean), ptr(var), ptr(n)))
        return mean[:self.FD], var[:self.FD], int(n[0])

    def flat_start_model(self, J, M, mean, var, coeff=None, logdet=False):
        """The flat-start model made on the device (AcousticModel.py:504-516): every mixture m of every one of the J states gets
        mean + coeff[m] * var, var and weight 1 / M; coeff (M,) or None (differentiation=False).  Afterwards the engine holds the
        model exactly as load_model of those (J, M, D) arrays would have left it."""
        mean, var = as_c(mean, np.float64).reshape(-1), as_c(var, np.float64).reshape(-1)
        if mean.shape != var.shape:
            raise ValueError('mean %s and var %s must be (D,)' % (mean.shape, var.shape))
        c = None
        if coeff is not None:
            c = as_c(coeff, np.float64).reshape(-1)
            if c.shape != (int(M),):
                raise ValueError('coeff must hold M = %d values, got %s' % (M, c.shape))
        self._check(self._lib.pcl_model_flat_start(self._ctx, int(J), int(M), mean.size, ptr(mean), ptr(var), ptr(c), 1 if logdet else 0))
        self.J, self.M, self.D = int(J), int(M), int(mean.size)
        self._model_key = None

    def flat_start(self, T, frame_begin, J, M, n_utts=None, step=1, coeff=None, logdet=False):
        """frames_moments + flat_start_model in one call, the moments going from the frames into the model on the device.
        Returns (mean, var, n_rows)."""
        T, fb = self._utt_ranges(T, frame_begin)
        c = None
        if coeff is not None:
            c = as_c(coeff, np.float64).reshape(-1)
            if c.shape != (int(M),):
                raise ValueError('coeff must hold M = %d values, got %s' % (M, c.shape))
        mean, var = np.empty(max(self.FD, 1)), np.empty(max(self.FD, 1))
        n = np.zeros(1, dtype=np.int64)
        self._check(self._lib.pcl_flat_start(self._ctx, T.size, ptr(T), ptr(fb), int(T.size if n_utts is None else n_utts), int(step), int(J),
                                             int(M), ptr(c), 1 if logdet else 0, ptr(mean), ptr(var), ptr(n)))
        self.J, self.M, self.D = int(J), int(M), self.FD
        self._model_key = None
        return mean[:self.FD], var[:self.FD], int(n[0])

    def mixup(self, M_new, perturb=0.2, want_origin=False):
        """Grow the resident model from M to M_new mixtures per state on the device (pcl_model_mixup): per state, rounds in which the
        heaviest mixtures with a weight > 0 are split -- parent and child share the halved weight and the variance, their means move
        apart by perturb * sqrt(var) -- until the state holds M_new.  Afterwards the engine holds the model exactly as load_model of
        the grown (J, M_new, D) arrays would have left it, with a zeroed statistics block; frames, unit transitions and live Segments
        stay.  want_origin=True: returns origin (J, M_new) int32, the old mixture every new one descends from."""
        M_new = int(M_new)
        origin = np.empty((self.J, M_new), dtype=np.int32) if want_origin and self.J > 0 and M_new > 0 else None
        self._check(self._lib.pcl_model_mixup(self._ctx, M_new, float(perturb), ptr(origin)))
        self.M = M_new
        self._model_key = None
        return origin if want_origin else None

    def uniform_segments(self, unit_ids, T, frame_begin, gmm_num, J, want_map=False):
        """Uniform segmentation of labelled utterances (multi_process_data(init=True): __eq_segment mode 'e', then __get_gmmdata,
        AcousticModel.py:605-644): every utterance is cut into equal chunks, one per label unit, every chunk into gmm_num slices.
        unit_ids as label_batch takes them; J = n_units * gmm_num.  Needs neither a model nor a unit inventory.  Returns the
        Segments of that map, built without it leaving the device (want_map=True: (Segments, frame_state (F,) int32))."""
        T, fb = self._utt_ranges(T, frame_begin)
        if isinstance(unit_ids, np.ndarray) and unit_ids.ndim == 2:
            lens = np.full(unit_ids.shape[0], unit_ids.shape[1], dtype=np.int32)
            flat = np.ascontiguousarray(unit_ids, dtype=np.int32).reshape(-1)
        else:
            lens = np.array([len(l) for l in unit_ids], dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in unit_ids] + [np.zeros(0, np.int32)]),
                                        dtype=np.int32)
        if lens.shape != T.shape:
            raise ValueError('labels and T must be equal-length')
        if flat.size == 0:
            flat = np.zeros(1, dtype=np.int32)
        state = np.empty(max(self.F, 1), dtype=np.int32) if want_map else None
        h = C.c_void_p()
        self._check(self._lib.pcl_uniform_segments(self._ctx, T.size, ptr(lens), ptr(flat), ptr(T), ptr(fb), int(gmm_num), int(J), ptr(state),
                                                   C.byref(h)))
        seg = Segments(self, None, int(J), handle=h)
        return (seg, state[:self.F]) if want_map else seg

    # ------------------------------------------------------------------ unit inventory, label-built batches
    def load_units(self, unit_trans):
        """unit_trans: (n_units, S, S) transition matrices (LHMM.transmat of every unit HMM, AcousticModel.py:174-181).
        Unit i owns GMM states i*(S-2) .. of the loaded model.  ln A is taken here with np.log, the values the
        reference's forward / Viterbi use (LHMM.py:340,571)."""
        t = as_c(unit_trans, np.float64)
        if t.ndim != 3 or t.shape[1] != t.shape[2]:
            raise ValueError('unit_trans must be (n_units, S, S)')
        with np.errstate(divide='ignore'):
            lt = np.ascontiguousarray(np.log(t))
        self._check(self._lib.pcl_units_upload(self._ctx, t.shape[0], t.shape[1], ptr(t), ptr(lt)))
        self.n_units, self.S = int(t.shape[0]), int(t.shape[1])

    def units_download(self):
        t = np.empty((self.n_units, self.S, self.S))
        self._check(self._lib.pcl_units_download(self._ctx, ptr(t)))
        return t

    def label_batch(self, unit_ids, T, frame_begin, tied=False):
        """Sentence HMMs of a list of labels (AcousticModel.embedded for every utterance at once, in the library).  tied=True: over the
        tied states of the resident tying (load_tying; pcl_batch_create_labels_tied) -- the model has the tying's J_t states, every label
        position's states come from a walk of the tree on the device, and the batch is a label-built batch for accumulate_hmm,
        refresh_transitions, align_segments, accumulate_tree and accumulate_lda."""
        return Batch(self, None, T, frame_begin, unit_ids=unit_ids, tied=tied)

    def load_tying(self, tree, n_states=None, n_roots=None):
        """Make a ContextTree.Tree's node arrays the resident tying (pcl_tying_upload), in place of the one before.  The unit inventory
        (load_units) must be the tree's: n_units units of P + 2 states.  n_states / n_roots: J_t and R0 where they are not the tree's own
        count of leaves and largest root."""
        qm, cand, child, state, root_of = tree.tying_arrays()
        jt = int(tree.n_states if n_states is None else n_states)
        if qm.ndim != 2 or qm.shape[1] != tree.n_units + 1 or child.shape != (cand.size, 2) or state.shape != cand.shape \
                or root_of.shape != (tree.n_units * tree.P,):
            raise ValueError('the tree\'s arrays do not fit together: q_member %s, node_cand %s, node_child %s, node_state %s, root_of %s'
                             % (qm.shape, cand.shape, child.shape, state.shape, root_of.shape))
        self._check(self._lib.pcl_tying_upload(self._ctx, tree.n_units, tree.P, int(qm.shape[0]), ptr(qm), int(cand.size), ptr(cand), ptr(child),
                                               ptr(state), int(tree.n_roots if n_roots is None else n_roots), ptr(root_of), jt))
        self.tying_P, self.tying_J = int(tree.P), jt

    def drop_tying(self):
        """Remove the resident tying (pcl_tying_drop).  Batches made over it keep their states."""
        self._check(self._lib.pcl_tying_drop(self._ctx))
        self.tying_P = self.tying_J = 0

    def tying_lookup(self, ctx3):
        """Tied states of arbitrary contexts, seen in training or not (pcl_tying_lookup; the device form of Tree.lookup): ctx3 (n, 3) int32
        = (left, centre, right) with n_units for "no neighbour" -> (n, P) int32."""
        c = as_c(ctx3, np.int32).reshape(-1, 3)
        P = int(getattr(self, 'tying_P', 0)) or max(int(getattr(self, 'S', 2)) - 2, 1)   # (without a tying the library refuses)
        out = np.empty((max(c.shape[0], 1), P), dtype=np.int32)
        self._check(self._lib.pcl_tying_lookup(self._ctx, int(c.shape[0]), ptr(c), ptr(out)))
        return out[:c.shape[0]]

    def load_lexicon(self, tree):
        """The flat pronunciation tree of Lexicon.PronunciationLexicon.compile (units = ids of the loaded inventory)."""
        nu = as_c(tree['node_units'], np.int32)
        nn = as_c(tree['node_nunits'], np.int32)
        if nu.shape != (len(nn), 2):                  # the device layout is [n_nodes][2] (PronunciationLexicon.compile(max_units=2))
            raise ValueError('tree node_units must be (n_nodes, 2), got %r' % (nu.shape,))
        cp = as_c(tree['child_ptr'], np.int32)
        ci = as_c(tree['child_idx'], np.int32) if len(tree['child_idx']) else np.zeros(1, dtype=np.int32)
        nw = as_c(tree['node_word'], np.int32)
        ro = as_c(tree['roots'], np.int32)
        self._check(self._lib.pcl_lexicon_upload(self._ctx, len(nn), ptr(nu), ptr(nn), ptr(cp), ptr(ci), ptr(nw), len(ro), ptr(ro)))
        self.n_nodes = len(nn)
        self._lex_tree = dict(node_units=nu.copy(), node_nunits=nn.copy(), child_ptr=cp.copy(), child_idx=ci[:int(cp[-1])].copy())

    def tie_lexicon(self, node_ctx=None):
        """Tied states of every (node, unit slot, state position) of the loaded pronunciation tree under the resident tying (load_tying;
        pcl_lexicon_tie), kept beside the tree for Batch.decode(tied=True): a snapshot, as for tied batches.  node_ctx (n_nodes, 2, 3)
        int32 = (left, centre, right); None: the default rule, PronunciationLexicon.node_contexts of the tree load_lexicon took."""
        if node_ctx is None:
            from .Lexicon.PronunciationLexicon import node_contexts
            tree = getattr(self, '_lex_tree', None)
            if tree is None:
                raise ValueError('tie_lexicon: no pronunciation tree (load_lexicon first)')
            node_ctx = node_contexts(tree, self.n_units)
        c = as_c(node_ctx, np.int32)
        if c.shape != (getattr(self, 'n_nodes', 0), 2, 3):
            raise ValueError('node_ctx must be (n_nodes, 2, 3) = (%d, 2, 3), got %r' % (getattr(self, 'n_nodes', 0), c.shape))
        self._check(self._lib.pcl_lexicon_tie(self._ctx, ptr(c)))
        self._lex_tie_P = int(self.tying_P)

    def untie_lexicon(self):
        """Remove the tree's tied states (pcl_lexicon_untie); nothing happens when there are none."""
        self._check(self._lib.pcl_lexicon_untie(self._ctx))

    def lexicon_states(self):
        """The kept tied states (pcl_lexicon_states): (n_nodes, 2 P) int32, -1 in the second slot of a one-unit node."""
        P = int(getattr(self, '_lex_tie_P', 0)) or max(int(getattr(self, 'S', 2)) - 2, 1)   # (not tied: the library refuses)
        out = np.empty((max(int(getattr(self, 'n_nodes', 0)), 1), 2 * P), dtype=np.int32)
        self._check(self._lib.pcl_lexicon_states(self._ctx, ptr(out)))
        return out[:self.n_nodes]

    def load_language_model(self, compiled):
        """The tables of LanguageModel.Ngram.compile (pre-scaled, ARPA-shaped; rule D6 in include/poccala_hip.h) for the loaded tree:
        Batch.decode(lm=True) then adds the bigram term where words end.  A new tree drops them."""
        uni, bow = as_c(compiled['uni'], np.float64), as_c(compiled['bow'], np.float64)
        rp = as_c(compiled['row_ptr'], np.int64)
        col, val = as_c(compiled['col'], np.int32), as_c(compiled['val'], np.float64)
        nwp, nwi = as_c(compiled['node_word_ptr'], np.int32), as_c(compiled['node_word_ids'], np.int32)
        if len(bow) != len(uni) or len(rp) != len(uni) + 1 or len(col) != len(val) or len(nwp) != self.n_nodes + 1:
            raise ValueError('language model tables do not fit together (W = %d, row_ptr %d, col %d, val %d, node_word_ptr %d for %d nodes)'
                             % (len(uni), len(rp), len(col), len(val), len(nwp), self.n_nodes))
        if len(rp) and int(rp[-1]) != len(col) or len(nwp) and int(nwp[-1]) != len(nwi):
            raise ValueError('language model tables: the last pointer entry is not the length of the list it points into')
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        self._check(self._lib.pcl_lm_upload(self._ctx, len(uni), ptr(uni), ptr(bow), ptr(rp), ptr(pad(col)), ptr(pad(val)), ptr(nwp), ptr(pad(nwi))))

    def all_state_batch(self, T, frame_begin):
        """Batch whose emission rows are [entry, every GMM state 0..J-1, exit]: what the decoder reads (BASELINE config 5:
        no label, every state of the inventory is scored for every frame)."""
        T = as_c(T, np.int32).reshape(-1)
        b = Batch(self, np.full(len(T), self.J + 2, dtype=np.int32), T, frame_begin)
        rows = np.concatenate([[PCL_ROW_ENTRY], np.arange(self.J), [PCL_ROW_EXIT]]).astype(np.int32)
        b.set_states([rows] * len(T))
        return b

    def hmm_acc_zero(self):
        self._check(self._lib.pcl_hmm_acc_zero(self._ctx))

    def hmm_acc_download(self):
        """(ksai_acc (n_units, S-2, S), gamma_acc (n_units, S-2)): log domain, -inf where nothing was added
        (LHMM.ksai_acc / LHMM.gamma_acc of every unit, merged over all label positions of all batches)."""
        ks = np.empty((self.n_units, self.S - 2, self.S))
        ga = np.empty((self.n_units, self.S - 2))
        self._check(self._lib.pcl_hmm_acc_download(self._ctx, ptr(ks), ptr(ga)))
        return ks, ga

    def mstep_transitions(self):
        """LHMM.update_param's transition update for every unit that occurred (LHMM.py:519-520)."""
        self._check(self._lib.pcl_mstep_transitions(self._ctx))

    # ------------------------------------------------------------------ E-step statistics
    def stats_zero(self):
        self._check(self._lib.pcl_stats_zero(self._ctx))

    def stats_download(self, moments=True):
        """Linear-domain sums: acc (J,M), alpha_acc (J,), and unless moments=False mean_acc (J,M,D), cov_acc (J,M,D)."""
        acc = np.empty((self.J, self.M))
        al = np.empty((self.J,))
        if not moments:
            self._check(self._lib.pcl_stats_download(self._ctx, ptr(acc), ptr(al), None, None))
            return dict(acc=acc, alpha_acc=al)
        me = np.empty((self.J, self.M, self.D))
        co = np.empty((self.J, self.M, self.D))
        self._check(self._lib.pcl_stats_download(self._ctx, ptr(acc), ptr(al), ptr(me), ptr(co)))
        return dict(acc=acc, alpha_acc=al, mean_acc=me, cov_acc=co)

    def accumulate_prune(self, log2_threshold):
        """Approximate mode of Batch.accumulate: leave out (frame, state) pairs with gamma_t(j) < 2^log2_threshold
        (default: only pairs that are exactly zero in the kernel's arithmetic)."""
        self._check(self._lib.pcl_accumulate_prune(self._ctx, float(log2_threshold)))

    def mstep(self, c_covariance=1e-3):
        """GMM.update_param for every state on the device (Clustering.py:682-693); rebuilds the scoring layouts."""
        self._check(self._lib.pcl_mstep(self._ctx, float(c_covariance)))
        self._model_key = None                       # the resident model is no longer what was uploaded

    # ------------------------------------------------------------------ speaker adaptation from the resident statistics
    def _state_class(self, state_class):
        if state_class is None:
            return None
        sc = as_c(state_class, np.int32).reshape(-1)
        if sc.shape != (self.J,):
            raise ValueError('state_class must hold one class per state (J = %d), got %s' % (self.J, sc.shape))
        return sc

    def mllr_estimate(self, state_class=None, n_classes=1, min_occ=1000.0):
        """MLLR mean transforms (pcl_mllr_estimate) from the statistics the last accumulate pass left: state_class (J,) int32 gives every
        state its regression class in [0, n_classes), -1 = leave the state alone, None = one class of all states.  Returns
        (W (R, D, D+1) -- column 0 the offset --, occ (R,), status (R,) int32: 0, or the reason a class was refused and got the
        identity: 1 occupancy below min_occ, 2 fewer than D+1 contributing mixtures, 3 a pivot not > 0).  The model is not changed;
        the transforms stay on the device for transform_means()."""
        R = int(n_classes)
        sc = self._state_class(state_class)
        n = max(R, 1)
        W, occ, status = np.empty((n, self.D, self.D + 1)), np.empty(n), np.empty(n, dtype=np.int32)
        self._check(self._lib.pcl_mllr_estimate(self._ctx, R, ptr(sc), float(min_occ), ptr(W), ptr(occ), ptr(status)))
        return W, occ, status

    def transform_means(self, W=None, state_class=None, n_classes=1):
        """mean <- A_r mean + b_r on the device (pcl_model_transform_means) for every state of class r >= 0, W[r] = [b_r | A_r]; W=None:
        the transforms of the last mllr_estimate, which never left the device.  Variances and weights stay; the scoring layouts are
        rebuilt as mstep() rebuilds them."""
        R = int(n_classes)
        sc = self._state_class(state_class)
        if W is not None:
            W = as_c(W, np.float64)
            if W.shape != (R, self.D, self.D + 1):
                raise ValueError('W must be (n_classes, D, D+1) = %s, got %s' % ((R, self.D, self.D + 1), W.shape))
        self._check(self._lib.pcl_model_transform_means(self._ctx, R, ptr(sc), ptr(W)))
        self._model_key = None

    def mstep_map(self, tau):
        """MAP re-estimation of the means (pcl_mstep_map): mean <- (tau mean + s) / (tau + acc) from the resident statistics for every
        mixture the data reached; tau = 0 is mstep()'s mean.  Variances and weights stay."""
        self._check(self._lib.pcl_mstep_map(self._ctx, float(tau)))
        self._model_key = None

    # ------------------------------------------------------------------ discriminative training: MMI by extended Baum-Welch
    def ebw_hold(self):
        """Keep the statistics accumulated so far as the NUMERATOR set of mstep_ebw() (pcl_ebw_hold): a second resident block; the live
        block keeps its bits, and is the caller's to clear (stats_zero) and fill with the denominator.  The held set goes with the model
        it was accumulated under: load_model, flat starts, mixup and every mstep*/transform_means drop it."""
        self._check(self._lib.pcl_ebw_hold(self._ctx))

    def ebw_drop(self):
        self._check(self._lib.pcl_ebw_drop(self._ctx))

    def ebw_stats(self):
        """stats_download() of the held numerator set."""
        acc, al = np.empty((self.J, self.M)), np.empty((self.J,))
        me, co = np.empty((self.J, self.M, self.D)), np.empty((self.J, self.M, self.D))
        self._check(self._lib.pcl_ebw_stats_download(self._ctx, ptr(acc), ptr(al), ptr(me), ptr(co)))
        return dict(acc=acc, alpha_acc=al, mean_acc=me, cov_acc=co)

    def mstep_ebw(self, E=2.0, tau=100.0, c_covariance=1e-3, weight_iters=100, want_D=False):
        """Extended Baum-Welch update of means, variances and weights (pcl_mstep_ebw): numerator = the set ebw_hold() kept, denominator =
        the live statistics, both accumulated under the current model.  D = max(E gd, 2 Dmin) per mixture, I-smoothing tau on the
        numerator, Povey's weight iteration.  Returns the counts dict(updated, kept, floored, weights_kept), and with want_D=True
        (counts, D (J, M)): the smoothing constant used, 0 for a mixture that kept its parameters."""
        D = np.empty((self.J, self.M)) if want_D else None
        counts = np.zeros(4, dtype=np.int64)
        self._check(self._lib.pcl_mstep_ebw(self._ctx, float(E), float(tau), float(c_covariance), int(weight_iters), ptr(D), ptr(counts)))
        self._model_key = None
        out = dict(zip(('updated', 'kept', 'floored', 'weights_kept'), (int(c) for c in counts)))
        return (out, D) if want_D else out

    def loop_batch(self, T, frame_begin, unit_trans, unit_prior=None, s=5):
        """A unit-loop denominator graph over the whole inventory, as a general batch: rows [entry, every state 0..J-1, exit] (as
        all_state_batch); unit i's emitting rows carry unit_trans[i][1:-1] inside their own block; the mass a row sends to its unit's
        exit column is spread over the FIRST emitting row of every unit in proportion to unit_prior (default uniform); the entry row
        goes to those first rows with unit_prior; pi is uniform 1/N, as embedded_structure makes it.  Dense (J+2)^2 matrices per
        utterance: for inventories of a few hundred states."""
        a, pi = loop_structure(unit_trans, unit_prior, s)
        if a.shape[0] != self.J + 2:
            raise ValueError('%d units of %d emitting states do not cover the model\'s %d states' % (len(unit_trans), s - 2, self.J))
        T = as_c(T, np.int32).reshape(-1)
        b = Batch(self, np.full(len(T), self.J + 2, dtype=np.int32), T, frame_begin)
        with np.errstate(divide='ignore'):
            la, lpi = np.log(a), np.log(pi)
        b.set_transitions([la] * b.U, [lpi] * b.U)
        rows = np.concatenate([[PCL_ROW_ENTRY], np.arange(self.J), [PCL_ROW_EXIT]]).astype(np.int32)
        b.set_states([rows] * b.U)
        return b

    # ------------------------------------------------------------------ fMLLR: per-speaker transforms of the resident frames
    def fmllr_zero(self, n_speakers):
        """Make (or clear) the context's fMLLR statistics for n_speakers speakers (pcl_fmllr_zero); a resident estimate is dropped."""
        self._check(self._lib.pcl_fmllr_zero(self._ctx, int(n_speakers)))
        self.fmllr_S = int(n_speakers)

    def fmllr_stats(self):
        """(G (S, D, D+1, D+1), k (S, D, D+1), beta (S,)): what Batch.accumulate_fmllr has summed since fmllr_zero."""
        S, D = int(getattr(self, 'fmllr_S', 0)), self.D
        n = max(S, 1)
        G, k, beta = np.empty((n, D, D + 1, D + 1)), np.empty((n, D, D + 1)), np.empty(n)
        self._check(self._lib.pcl_fmllr_stats_download(self._ctx, ptr(G), ptr(k), ptr(beta)))
        return G[:S], k[:S], beta[:S]

    def fmllr_estimate(self, n_iter=20, min_occ=1000.0):
        """One transform W[s] = [b | A] per speaker from the resident statistics (pcl_fmllr_estimate; the rule: include/poccala_hip.h):
        (W (S, D, D+1), logdet (S,) = ln|det A|, q_trace (S, n_iter) = the auxiliary value after every sweep, status (S,) int32: 0, or why
        the speaker was refused and got [0 | I]: 1 occupancy below min_occ, 2 a G not positive definite, 3 a singular step).  The
        transforms stay on the device for transform_frames()."""
        S, D, K = max(int(getattr(self, 'fmllr_S', 0)), 1), self.D, max(int(n_iter), 1)
        W, logdet, q, status = np.empty((S, D, D + 1)), np.empty(S), np.empty((S, K)), np.empty(S, dtype=np.int32)
        self._check(self._lib.pcl_fmllr_estimate(self._ctx, int(n_iter), float(min_occ), ptr(W), ptr(logdet), ptr(q), ptr(status)))
        return W, logdet, q, status

    def transform_frames(self, T, frame_begin, utt_speaker, W=None, n_speakers=None):
        """y = b + A x in place on the resident frame matrix (pcl_frames_transform) for the rows [frame_begin[u], + T[u]) of every
        utterance whose utt_speaker[u] >= 0; W (S, D, D+1) or None = the transforms of the last fmllr_estimate.  Speakers whose W is
        [0 | I] and rows outside the utterances keep their bits.  Batches scored before the call keep their old emissions."""
        T, fb = self._utt_ranges(T, frame_begin)
        spk = as_c(utt_speaker, np.int32).reshape(-1)
        if fb is None or spk.shape != T.shape:
            raise ValueError('T, frame_begin and utt_speaker must be equal-length')
        if W is not None:
            W = as_c(W, np.float64)
            if W.ndim != 3 or W.shape[1:] != (self.FD, self.FD + 1):
                raise ValueError('W must be (n_speakers, D, D+1) with D = %d, got %s' % (self.FD, W.shape))
        S = int(n_speakers) if n_speakers is not None else (W.shape[0] if W is not None else int(getattr(self, 'fmllr_S', 0)))
        self._check(self._lib.pcl_frames_transform(self._ctx, T.size, ptr(T), ptr(fb), ptr(spk), S, ptr(W)))
        self._frames_key = None                      # the resident frames are no longer what was uploaded

    # ------------------------------------------------------------------ MLLT: one square transform of the features for the whole corpus
    def mllt_zero(self, state_keep=None):
        """Make (or clear) the context's MLLT statistics for the resident model (pcl_mllt_zero): state_keep (J,), 0 = the state -- silence,
        say -- is left out of both sides of G; None = every state counts."""
        sk = None
        if state_keep is not None:
            sk = as_c(np.asarray(state_keep) != 0, np.int32).reshape(-1)
            if sk.shape != (self.J,):
                raise ValueError('state_keep must hold one entry per state (J = %d), got %s' % (self.J, sk.shape))
        self._check(self._lib.pcl_mllt_zero(self._ctx, ptr(sk)))

    def mllt_stats(self):
        """(F (D, D, D), beta): the frame side of G and its occupancy, what Batch.accumulate_mllt has summed since mllt_zero."""
        D = self.D
        F, beta = np.empty((D, D, D)), np.empty(1)
        self._check(self._lib.pcl_mllt_stats_download(self._ctx, ptr(F), ptr(beta)))
        return F, float(beta[0])

    def mllt_estimate(self, n_iter=20, min_occ=1000.0):
        """The MLLT matrix from the resident statistics (pcl_mllt_estimate; the rule: include/poccala_hip.h): G_i = F_i - C_i with the
        mixture side C_i from the E-step statistics block and the model, then n_iter row sweeps from A = I.  Returns a dict: A (D, D),
        logdet = ln|det A|, q_trace (n_iter + 1,) = the auxiliary value at A = I and after every sweep, G (D, D, D), occ = (beta of
        the frames, sum of acc over the kept contributing mixtures), status: 0, or why the estimate was refused and A = I: 1 beta
        below min_occ, 2 a G_i not positive definite, 3 a singular step.  Neither the model nor the frames are changed: apply A with
        transform_frames(T, begin, zeros, W) and transform_means(W), W = [0 | A][None]."""
        D, K = self.D, max(int(n_iter), 1) + 1
        A, logdet, q, G, occ, status = np.empty((D, D)), np.empty(1), np.empty(K), np.empty((D, D, D)), np.empty(2), np.empty(1, dtype=np.int32)
        self._check(self._lib.pcl_mllt_estimate(self._ctx, int(n_iter), float(min_occ), ptr(A), ptr(logdet), ptr(q), ptr(G), ptr(occ), ptr(status)))
        return dict(A=A, logdet=float(logdet[0]), q_trace=q, G=G, occ=occ, status=int(status[0]))

    # ------------------------------------------------------------------ LDA: class statistics of spliced frames, projection to a new width
    def lda_zero(self, n_classes, left, right):
        """Make (and clear) the context's LDA class statistics (pcl_lda_zero) for n_classes classes and the splice context (left, right)
        at the dimension of the resident frames: per class the rows, sum x and sum x x^T of the spliced vectors x."""
        self._check(self._lib.pcl_lda_zero(self._ctx, int(n_classes), int(left), int(right)))
        self._lda = (int(n_classes), int(left), int(right), (int(left) + int(right) + 1) * int(self.FD))

    def lda_accumulate(self, T, frame_begin, frame_class):
        """Add the rows [frame_begin[u], + T[u]) of the resident frames to the statistics (pcl_lda_accumulate): frame_class (F,) int32, one
        class in [0, n_classes) per row of the frame matrix, -1 = skip the row.  A row is spliced inside its own utterance."""
        T, fb = self._utt_ranges(T, frame_begin)
        cls = as_c(frame_class, np.int32).reshape(-1)
        if fb is None or cls.shape != (int(self.F),):
            raise ValueError('frame_begin is needed and frame_class must hold one class per frame row (F = %d), got %s' % (self.F, cls.shape))
        self._check(self._lib.pcl_lda_accumulate(self._ctx, T.size, ptr(T), ptr(fb), ptr(cls)))

    def lda_stats(self):
        """(n (R,), s (R, Ds), S (R, Ds, Ds)) float64: what lda_accumulate / Batch.accumulate_lda have summed since lda_zero."""
        R, _, _, Ds = getattr(self, '_lda', (0, 0, 0, 0))
        r, d = max(R, 1), max(Ds, 1)
        n, s, S = np.empty(r), np.empty((r, d)), np.empty((r, d, d))
        self._check(self._lib.pcl_lda_stats_download(self._ctx, ptr(n), ptr(s), ptr(S)))
        return n[:R], s[:R, :Ds], S[:R, :Ds, :Ds]

    def lda_estimate(self, D_out, eps=1e-10):
        """The LDA transform from the resident statistics, on the host in float64 (the rule: include/poccala_hip.h, ESTIMATE): within-class
        covariance W (floored by eps trace(W) / Ds on the diagonal) = L L^T, the D_out leading eigenvectors V of L^-1 B L^-T, A = V^T L^-1,
        b = -A m, every row's largest-magnitude entry made positive.  Returns (A (D_out, Ds), b (D_out,), eigenvalues (D_out,) descending);
        the projected data has zero mean and unit within-class covariance."""
        n, s, S = self.lda_stats()
        Ds, D_out = s.shape[1], int(D_out)
        live = np.flatnonzero(n > 0)
        if D_out < 1 or D_out > Ds:
            raise ValueError('lda_estimate: D_out = %d, need 1 .. the spliced dimension %d' % (D_out, Ds))
        if live.size == 0:
            raise ValueError('lda_estimate: the statistics are empty')
        N = n[live].sum()
        m = s[live].sum(axis=0) / N
        W, B = np.zeros((Ds, Ds)), np.zeros((Ds, Ds))
        for r in live:
            W += S[r] - np.outer(s[r], s[r]) / n[r]
            d = s[r] / n[r] - m
            B += n[r] * np.outer(d, d)
        W, B = W / N, B / N
        W = 0.5 * (W + W.T)
        W[np.diag_indices(Ds)] += float(eps) * np.trace(W) / Ds
        L = np.linalg.cholesky(W)
        Li = np.linalg.solve(L, np.eye(Ds))
        M = Li.dot(B).dot(Li.T)
        lam, V = np.linalg.eigh(0.5 * (M + M.T))
        top = np.argsort(-lam, kind='stable')[:D_out]
        A = V[:, top].T.dot(Li)
        b = -A.dot(m)
        flip = A[np.arange(D_out), np.abs(A).argmax(axis=1)] < 0
        A[flip], b[flip] = -A[flip], -b[flip]
        return np.ascontiguousarray(A), b, lam[top]

    def splice_project(self, T, frame_begin, left, right, A, b):
        """The resident (F, D) frames become (F, D_out): y = b + A x over the spliced vector x (context (left, right), edge replication
        inside the utterance) of every row of the listed utterances, rows of no utterance zero (pcl_frames_splice_project).  A (D_out,
        (left + right + 1) D), b (D_out,).  Refused while a Batch or Segments made on the old frames is open."""
        T, fb = self._utt_ranges(T, frame_begin)
        A, b = as_c(A, np.float64), as_c(b, np.float64).reshape(-1)
        Ds = (int(left) + int(right) + 1) * int(self.FD)
        if fb is None or A.ndim != 2 or A.shape[1] != Ds or b.shape != (A.shape[0],):
            raise ValueError('frame_begin is needed, A must be (D_out, %d) and b (D_out,), got %s and %s' % (Ds, A.shape, b.shape))
        self._check(self._lib.pcl_frames_splice_project(self._ctx, T.size, ptr(T), ptr(fb), int(left), int(right), A.shape[0], ptr(A), ptr(b)))
        self.FD = int(A.shape[0])
        self._frames_key = None                      # the resident frames are no longer what was uploaded

    # ------------------------------------------------------------------ phonetic decision tree: context statistics, tied states
    def tree_zero(self, n_rows):
        """Make (and clear) the context's decision-tree statistics for n_rows = E * P rows at the dimension of the resident frames
        (pcl_tree_zero): per row the frames n, sum x and sum x^2."""
        self._check(self._lib.pcl_tree_zero(self._ctx, int(n_rows)))

    def _tree_shape(self):
        """(R, D) of the context's decision-tree statistics (pcl_tree_stats_shape), (0, 0) when it holds none: asked of the context, so
        that a pcl_tree_zero made through the C-ABI on it is seen."""
        R, D = C.c_int32(), C.c_int32()
        self._check(self._lib.pcl_tree_stats_shape(self._ctx, C.byref(R), C.byref(D)))
        return int(R.value), int(D.value)

    def tree_accumulate(self, T, frame_begin, frame_row):
        """Add the rows [frame_begin[u], + T[u]) of the resident frames to the statistics (pcl_tree_accumulate): frame_row (F,) int32, the
        statistics row in [0, n_rows) of every row of the frame matrix, -1 = skip the row."""
        T, fb = self._utt_ranges(T, frame_begin)
        rows = as_c(frame_row, np.int32).reshape(-1)
        if fb is None or rows.shape != (int(self.F),):
            raise ValueError('frame_begin is needed and frame_row must hold one row per frame row (F = %d), got %s' % (self.F, rows.shape))
        self._check(self._lib.pcl_tree_accumulate(self._ctx, T.size, ptr(T), ptr(fb), ptr(rows)))

    def tree_stats(self):
        """(n (R,) int64, s (R, D), q (R, D)): what tree_accumulate / Batch.accumulate_tree have summed since tree_zero."""
        R, D = self._tree_shape()
        n, s, q = np.empty(max(R, 1), dtype=np.int64), np.empty((max(R, 1), max(D, 1))), np.empty((max(R, 1), max(D, 1)))
        self._check(self._lib.pcl_tree_stats_download(self._ctx, ptr(n), ptr(s), ptr(q)))
        return n[:R], s[:R, :D], q[:R, :D]

    def tree_stats_load(self, n, s, q):
        """Replace the resident statistics (pcl_tree_stats_upload): n (R,) int64, s and q (R, D), the shapes of the last tree_zero."""
        R, D = self._tree_shape()
        n, s, q = as_c(n, np.int64).reshape(-1), as_c(s, np.float64), as_c(q, np.float64)
        if n.shape != (R,) or s.shape != (R, D) or q.shape != (R, D):
            raise ValueError('the statistics are n (%d,), s and q (%d, %d), got %s, %s, %s' % (R, R, D, n.shape, s.shape, q.shape))
        self._check(self._lib.pcl_tree_stats_upload(self._ctx, ptr(n), ptr(s), ptr(q)))

    def tree_build(self, event_ctx, P, n_units, q_member, root_of, n_roots=None, min_count=1, min_gain=0.0, max_leaves=None, var_floor=1e-4,
                   install=False, logdet=False):
        """Grow the trees over the resident statistics (pcl_tree_build; the rule: include/poccala_hip.h) and return the ContextTree.Tree.
        event_ctx (E, 3) int32, q_member (Q, n_units + 1) uint8, root_of (n_units * P,) int32.  install=True: the resident model becomes
        the (J_t, 1, D) one-Gaussian-per-leaf model, as flat_start_model would have left it."""
        from .AcousticModel.ContextTree import Tree
        ec = as_c(event_ctx, np.int32).reshape(-1, 3)
        qm = as_c(q_member, np.uint8)
        ro = as_c(root_of, np.int32).reshape(-1)
        P, n_units = int(P), int(n_units)
        if qm.ndim != 2 or qm.shape[1] != n_units + 1 or ro.shape != (n_units * P,):
            raise ValueError('q_member must be (Q, %d) and root_of (%d,), got %s and %s' % (n_units + 1, n_units * P, qm.shape, ro.shape))
        E, Q = int(ec.shape[0]), int(qm.shape[0])
        R, D = E * P, self._tree_shape()[1]
        R0 = int(ro.max()) + 1 if n_roots is None else int(n_roots)
        ml = max(R0, R) if max_leaves is None else min(int(max_leaves), max(R0, R, 1))
        cap = max(R0 + 2 * max(ml - R0, 0), 1)
        node_cand, node_child, node_state = np.empty(cap, dtype=np.int32), np.empty((cap, 2), dtype=np.int32), np.empty(cap, dtype=np.int32)
        node_n, gain, row_state = np.empty(cap, dtype=np.int64), np.empty(cap), np.empty(max(R, 1), dtype=np.int32)
        leaf_n, leaf_s, leaf_q = np.empty(cap, dtype=np.int64), np.empty((cap, max(D, 1))), np.empty((cap, max(D, 1)))
        nn, ns = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        self._check(self._lib.pcl_tree_build(self._ctx, E, P, ptr(ec), n_units, Q, ptr(qm), R0, ptr(ro), int(min_count), float(min_gain), ml,
                                             float(var_floor), 1 if install else 0, 1 if logdet else 0, ptr(node_cand), ptr(node_child),
                                             ptr(node_state), ptr(node_n), ptr(gain), ptr(row_state), ptr(leaf_n), ptr(leaf_s), ptr(leaf_q),
                                             ptr(nn), ptr(ns)))
        N, Jt = int(nn[0]), int(ns[0])
        if install:
            self.J, self.M, self.D = Jt, 1, D
            self._model_key = None
        return Tree(P, n_units, node_cand=node_cand[:N].copy(), node_child=node_child[:N].copy(), node_state=node_state[:N].copy(),
                    node_n=node_n[:N].copy(), split_gain=gain[:(N - R0) // 2].copy(), row_state=row_state[:R].copy(), event_ctx=ec, q_member=qm,
                    root_of=ro, leaf_n=leaf_n[:Jt].copy(), leaf_s=leaf_s.reshape(-1)[:Jt * D].reshape(Jt, D).copy(),
                    leaf_q=leaf_q.reshape(-1)[:Jt * D].reshape(Jt, D).copy())

    # ------------------------------------------------------------------ CMVN: mean and variance normalisation of the resident frames
    def cmvn_zero(self, n_speakers):
        """Make (and clear) the context's CMVN statistics for n_speakers speakers at the dimension of the resident frames (pcl_cmvn_zero)."""
        self._check(self._lib.pcl_cmvn_zero(self._ctx, int(n_speakers)))
        self._cmvn = (int(n_speakers), int(self.FD))

    def _cmvn_args(self, T, frame_begin, utt_speaker):
        T, fb = self._utt_ranges(T, frame_begin)
        spk = as_c(np.arange(T.size) if utt_speaker is None else utt_speaker, np.int32).reshape(-1)
        if fb is None or spk.shape != T.shape:
            raise ValueError('T, frame_begin and utt_speaker must be equal-length')
        return T, fb, spk

    def cmvn_accumulate(self, T, frame_begin, utt_speaker=None):
        """Add the rows [frame_begin[u], + T[u]) of the resident frames to the statistics of speaker utt_speaker[u] (pcl_cmvn_accumulate);
        -1 = the utterance is skipped, None = every utterance its own speaker."""
        T, fb, spk = self._cmvn_args(T, frame_begin, utt_speaker)
        self._check(self._lib.pcl_cmvn_accumulate(self._ctx, T.size, ptr(T), ptr(fb), ptr(spk)))

    def cmvn_stats(self):
        """(n (S,) int64, s (S, D), q (S, D)): per speaker the rows, sum x and sum x^2 that cmvn_accumulate has summed since cmvn_zero."""
        S, D = getattr(self, '_cmvn', (0, 0))
        n, s, q = np.empty(max(S, 1), dtype=np.int64), np.empty((max(S, 1), max(D, 1))), np.empty((max(S, 1), max(D, 1)))
        self._check(self._lib.pcl_cmvn_stats_download(self._ctx, ptr(n), ptr(s), ptr(q)))
        return n[:S], s[:S, :D], q[:S, :D]

    def cmvn_apply(self, T, frame_begin, utt_speaker=None, norm_vars=True, var_floor=1e-20, min_count=1, n_speakers=None):
        """y = (x - m) / sqrt(v) (norm_vars) or x - m in place on the resident frames, per speaker from the resident statistics
        (pcl_frames_cmvn; the rule: include/poccala_hip.h).  Returns the (S,) int32 statuses: 0, or why the speaker's utterances were
        left as they were: 1 fewer than min_count rows, 2 a sum that is not finite.  Batches scored before the call keep their old
        emissions."""
        T, fb, spk = self._cmvn_args(T, frame_begin, utt_speaker)
        S = int(n_speakers) if n_speakers is not None else int(getattr(self, '_cmvn', (0, 0))[0])
        status = np.zeros(max(S, 1), dtype=np.int32)
        self._check(self._lib.pcl_frames_cmvn(self._ctx, T.size, ptr(T), ptr(fb), ptr(spk), S, 1 if norm_vars else 0, float(var_floor),
                                              int(min_count), ptr(status)))
        self._frames_key = None                      # the resident frames are no longer what was uploaded
        return status[:S]

    def cmvn_sliding(self, T, frame_begin, window=600, min_window=100, center=False, norm_vars=False, var_floor=1e-20):
        """Sliding-window CMVN in place on the resident frames (pcl_frames_cmvn_sliding): frame t is normalised by the mean (and variance)
        of a window of `window` rows of its own utterance -- centred on t, or the rows up to t (at least min_window of them where the
        utterance has as many) -- taken from the rows as they were before the call."""
        T, fb = self._utt_ranges(T, frame_begin)
        if fb is None:
            raise ValueError('frame_begin is needed')
        self._check(self._lib.pcl_frames_cmvn_sliding(self._ctx, T.size, ptr(T), ptr(fb), int(window), int(min_window), 1 if center else 0,
                                                      1 if norm_vars else 0, float(var_floor)))
        self._frames_key = None

    def frames_download(self, dtype=np.float64):
        """The resident frames as held, (F, D): np.float64 = the float64 copy (an error when the frames were uploaded as float32 and no
        copy exists), np.float32 = the float32 rows every default-precision kernel reads."""
        out = np.empty((max(int(self.F), 1), max(int(self.FD), 1)), dtype=np.float32 if np.dtype(dtype) == np.float32 else np.float64)
        if out.dtype == np.float32:
            self._check(self._lib.pcl_frames_download(self._ctx, None, ptr(out)))
        else:
            self._check(self._lib.pcl_frames_download(self._ctx, ptr(out), None))
        return out[:int(self.F), :int(self.FD)]

    def model_download(self):
        """(mean (J,M,D), var (J,M,D), weight (J,M)) float64 master copy."""
        mean = np.empty((self.J, self.M, self.D))
        var = np.empty((self.J, self.M, self.D))
        w = np.empty((self.J, self.M))
        self._check(self._lib.pcl_model_download(self._ctx, ptr(mean), ptr(var), ptr(w)))
        return mean, var, w

    def model_conditioning(self):
        """(cond (J,) float32, cond_max): conditioning of the centred expansion per state; states above cond_max
        are scored and accumulated by the direct-form kernels instead of the matrix-core ones."""
        cond = np.empty(self.J, dtype=np.float32)
        cmax = np.empty(1, dtype=np.float32)
        self._check(self._lib.pcl_model_conditioning(self._ctx, ptr(cond), ptr(cmax)))
        return cond, float(cmax[0])

    def score_occupancy(self, workgroups_per_cu):
        """0: the scoring kernel fills the CUs (default); 2: it leaves a third of each CU's registers to kernels of other streams
        (the streamed decoder's token passing).  Same results either way."""
        self._check(self._lib.pcl_score_occupancy(self._ctx, int(workgroups_per_cu)))

    def model_split_info(self):
        """(n_off (J,) int32, limit): mixtures per state that are off the matrix-core path (their own conditioning is beyond
        cond_max; the direct-form kernels evaluate them and the parts are merged); a state with more than `limit` of them
        leaves the matrix cores as a whole."""
        n_off = np.empty(self.J, dtype=np.int32)
        lim = np.empty(1, dtype=np.int32)
        self._check(self._lib.pcl_model_split_info(self._ctx, ptr(n_off), ptr(lim)))
        return n_off, int(lim[0])

    def coarse_pairs(self, reset=True):
        """(frame, mixture) pairs of off-pipe mixtures evaluated exactly since the last reset (counted under PCL_COARSE_STATS=1)."""
        n = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.pcl_coarse_counter(self._ctx, ptr(n), 1 if reset else 0))
        return int(n[0])

    def coarse_counters(self, reset=True):
        """(pairs evaluated exactly, tiles the coarse pass gave up and the direct-form subset kernel rescored) since the last reset
        (counted under PCL_COARSE_STATS=1)."""
        n, g = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
        self._check(self._lib.pcl_coarse_counters(self._ctx, ptr(n), ptr(g), 1 if reset else 0))
        return int(n[0]), int(g[0])

    # ------------------------------------------------------------------ RCCL
    def comm_unique_id(self):
        buf = np.zeros(128, dtype=np.uint8)
        rc = self._lib.pcl_comm_unique_id(ptr(buf))
        if rc != 0:
            raise PoccalaHipError(rc, self._lib.pcl_last_error(None).decode())
        return buf.tobytes()

    def comm_init(self, rank, nranks, unique_id):
        """ncclCommInitRank.  RCCL prints a version banner with C stdio on stdout; a caller that owes its parent
        exactly one line of stdout (bench.py) would see it arrive AFTER its own output when libc flushes at exit, so
        file descriptor 1 points at stderr while the communicator is created."""
        import ctypes, os, sys
        buf = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        libc = ctypes.CDLL(None)
        sys.stdout.flush()
        libc.fflush(None)
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            rc = self._lib.pcl_comm_init(self._ctx, int(rank), int(nranks), ptr(buf))
            libc.fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        self._check(rc)

    def comm_init_host(self, rank, nranks, allgather_bytes):
        """Rehearsal transport for several ranks on ONE device (RCCL refuses duplicate devices): `allgather_bytes(b)`
        returns every rank's bytes in rank order (poccala_amd.distributed.Control.allgather_bytes)."""
        def cb(user, send, nbytes, recv_all):
            try:
                parts = allgather_bytes(C.string_at(send, nbytes))
                if len(parts) != nranks or any(len(x) != nbytes for x in parts):
                    return 1
                C.memmove(recv_all, b''.join(parts), nbytes * nranks)
                return 0
            except Exception:          # never let an exception cross the C boundary
                return 2
        self._host_cb = _lib.ALLGATHER_FN(cb)       # keep the thunk alive as long as the context
        self._check(self._lib.pcl_comm_init_host(self._ctx, int(rank), int(nranks), self._host_cb, None))

    def comm_info(self):
        r, n, t, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.pcl_comm_info(self._ctx, C.byref(r), C.byref(n), C.byref(t), C.byref(c)))
        return dict(rank=r.value, nranks=n.value, transport={0: 'none', 1: 'rccl', 2: 'host-rehearsal'}[t.value], rccl_nranks=c.value)

    def pipe_info(self):
        """(chunks, released_early) of the last accumulate_exchange: how many state chunks left for the exchange while the pass still ran."""
        k, e = C.c_int(), C.c_int()
        self._check(self._lib.pcl_pipe_info(self._ctx, C.byref(k), C.byref(e)))
        return k.value, e.value

    def stats_allreduce(self):
        self._check(self._lib.pcl_stats_allreduce(self._ctx))

    def wire_payload(self):
        """The cheaper wire format of the E-step exchange for callers that opt in (bench.py --payload auto): float32 as soon as there is
        a wire (the 1.94 GB of statistics and the model cross xGMI as f32, half the bytes; every rank continues
        from the same rounded model; mean_acc travels as mean_acc - (bias + c_j) acc so that the rounding is not amplified), float64
        on one rank.  NOT the default: with it the re-estimated model depends on the world size."""
        return PCL_F32 if self.comm_info()['nranks'] > 1 else PCL_F64

    def accumulate_exchange_idle(self, c_covariance=1e-3, payload=PCL_F64, update_transitions=False, n_chunks=8):
        """Batch.accumulate_exchange for a rank that has no batch for this last pass (the others do): the same chunk exchanges, in the
        same order, on whatever this rank's statistics hold."""
        self._check(self._lib.pcl_accumulate_exchange_idle(self._ctx, float(c_covariance), int(payload), 1 if update_transitions else 0, int(n_chunks)))
        self._model_key = None

    def em_exchange(self, c_covariance=1e-3, payload=PCL_F64, update_transitions=False):
        """reduce-scatter of the statistics by state range -> M-step on the owned states -> all-gather of the model
        (+ merge of the per-unit HMM accumulators, + the transition update on request).  One rank: the M-step.
        payload: PCL_F64 (default: the reference's reducer is float64, LHMM.py:256-290 / Clustering.py:314-367, and the model then
        does not depend on the world size) or PCL_F32 (half the bytes on the wire; `wire_payload()` picks it when there is a wire)."""
        self._check(self._lib.pcl_em_exchange(self._ctx, float(c_covariance), int(payload), 1 if update_transitions else 0))
        self._model_key = None


class Lattice(object):
    """One utterance's word lattice (Batch.lattice): plain arrays, documented there."""
    __slots__ = ('frame', 'tok', 'node', 'hist', 'score', 'term', 'word', 'start', 'end', 'span', 'hist_frame', 'hist_seed', 'n_entries',
                 'n_arcs_wanted', 'overflow')


class Batch(object):
    """U sentence HMMs.  N[u] states, T[u] frames; matrices cross the boundary in the reference's
    (N,T) float64 layout, one array per utterance."""

    def __init__(self, engine, N, T, frame_begin=None, unit_ids=None, tied=False):
        self.eng = engine
        self._lib = engine._lib
        self.T = as_c(T, np.int32).reshape(-1)
        self._b = C.c_void_p()
        if unit_ids is not None:
            # label-built: N_u = (S-2) L_u + 2 (AcousticModel.py:966); structure built by pcl_batch_create_labels (tied: ..._labels_tied)
            if isinstance(unit_ids, np.ndarray) and unit_ids.ndim == 2:      # equal-length labels as one (U, L) array: no per-utterance Python
                lens = np.full(unit_ids.shape[0], unit_ids.shape[1], dtype=np.int32)
                flat = np.ascontiguousarray(unit_ids, dtype=np.int32).reshape(-1)
            else:
                lens = np.array([len(l) for l in unit_ids], dtype=np.int32)
                flat = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in unit_ids]), dtype=np.int32)
            self.N = ((engine.S - 2) * lens + 2).astype(np.int32)
            if self.N.shape != self.T.shape or self.N.size == 0 or frame_begin is None:
                raise ValueError('labels, T and frame_begin must be equal-length, non-empty')
            self.U = int(self.N.size)
            fb = as_c(frame_begin, np.int64).reshape(-1)
            logpi = np.ascontiguousarray(np.log(1.0 / self.N.astype(np.float64)))     # np.log(np.ones(N) / N), AcousticModel.py:1005
            self.label_len, self.labels = lens, flat
            create = self._lib.pcl_batch_create_labels_tied if tied else self._lib.pcl_batch_create_labels
            engine._check(create(engine._ctx, self.U, ptr(lens), ptr(flat), ptr(self.T), ptr(fb), ptr(logpi), C.byref(self._b)))
        else:
            self.N = as_c(N, np.int32).reshape(-1)
            if self.N.shape != self.T.shape or self.N.size == 0:
                raise ValueError('N and T must be equal-length, non-empty')
            if tied:
                raise ValueError('tied=True needs labels (unit_ids)')
            self.U = int(self.N.size)
            fb = None if frame_begin is None else as_c(frame_begin, np.int64).reshape(-1)
            engine._check(self._lib.pcl_batch_create(engine._ctx, self.U, ptr(self.N), ptr(self.T), ptr(fb),
                                                     C.byref(self._b)))
        self.tied = bool(tied)
        engine._batches.add(self)
        self._frame_begin = None if frame_begin is None else fb.copy()
        self._fetch_slots = set()                     # engine result slots with un-waited copies of this batch (fetch_async)
        n64, t64 = self.N.astype(np.int64), self.T.astype(np.int64)
        self._nt_off = np.concatenate([[0], np.cumsum(n64 * t64)])
        self._nn_off = np.concatenate([[0], np.cumsum(n64 * n64)])
        self._n_off = np.concatenate([[0], np.cumsum(n64)])
        self._t_off = np.concatenate([[0], np.cumsum(t64)])
        self._nnz_off = None
        self.nz_index = None

    def close(self):
        if getattr(self, '_b', None):
            if getattr(self.eng, '_ctx', None):       # the context frees its batches when it closes
                if getattr(self, '_fetch_slots', None):       # copies into an engine slot nobody waited for: the slot's next user must not race them
                    self._lib.pcl_batch_fetch_wait(self._b)
                    self._fetch_slots.clear()
                self._lib.pcl_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        self.eng._check(rc)

    def _ragged(self, arrays, shape_of, dtype=np.float64):
        out = []
        for u, a in enumerate(arrays):
            a = np.asarray(a, dtype=dtype)
            if a.shape != shape_of(u):
                raise ValueError('utterance %d: expected shape %s, got %s' % (u, shape_of(u), a.shape))
            out.append(a.reshape(-1))
        if len(out) != self.U:
            raise ValueError('expected %d arrays, got %d' % (self.U, len(out)))
        return np.ascontiguousarray(np.concatenate(out), dtype=dtype)

    # ------------------------------------------------------------------ inputs
    def set_transitions(self, logA, logpi):
        """logA[u] (N,N) = np.log(transmat), logpi[u] (N,) = np.log(pi) -- logged by the caller so that
        Viterbi sees bit-identical operands (LHMM.py:571,577)."""
        a = self._ragged(logA, lambda u: (self.N[u], self.N[u]))
        p = self._ragged(logpi, lambda u: (self.N[u],))
        # stored transitions (ln A > -inf) per utterance, row-major: the order of get('ksai_nz')
        self.nz_index = [np.nonzero(~np.isneginf(np.asarray(m, dtype=np.float64))) for m in logA]
        self._nnz_off = np.concatenate([[0], np.cumsum([len(ix[0]) for ix in self.nz_index])])
        self._check(self._lib.pcl_batch_set_transitions(self._b, ptr(a), ptr(p)))

    def set_states(self, row_state):
        s = self._ragged(row_state, lambda u: (self.N[u],), dtype=np.int32)
        self._check(self._lib.pcl_batch_set_states(self._b, ptr(s)))

    def set_emissions(self, B):
        b = self._ragged(B, lambda u: (self.N[u], self.T[u]))
        self._check(self._lib.pcl_batch_set_emissions(self._b, ptr(b)))

    def set_posteriors(self, lgamma):
        """ln gamma_t(i) per utterance (N,T), for accumulate() without a forward-backward on this batch."""
        g = self._ragged(lgamma, lambda u: (self.N[u], self.T[u]))
        self._check(self._lib.pcl_batch_set_posteriors(self._b, ptr(g)))

    # ------------------------------------------------------------------ kernels
    def score(self, precision=PCL_F32):
        self._check(self._lib.pcl_batch_score(self._b, int(precision)))

    def forward_backward(self, fix_pi=False, threshold=0.64):
        self._check(self._lib.pcl_batch_forward_backward(self._b, 1 if fix_pi else 0, float(threshold)))

    def viterbi(self, end_state_back=False):
        self._check(self._lib.pcl_batch_viterbi(self._b, 1 if end_state_back else 0))

    # ------------------------------------------------------------------ minimum Bayes risk: sMBR / MPFE, and MMI with an acoustic scale
    def mbr(self, frame_ref, kappa=1.0, group=1):
        """One forward-backward under the acoustic scale kappa with the expected frame accuracy against frame_ref (pcl_batch_mbr; the rule:
        include/poccala_hip.h).  frame_ref[u] (T_u,) int32: the reference state of every frame in [0, J), or -1 (ref_states() of the
        numerator batch gives it).  group = 1 compares states (sMBR), group = S - 2 units (MPFE).  Needs transitions, states and emissions,
        not forward_backward(); leaves everything get() returns as it was."""
        r = self._ragged(frame_ref, lambda u: (self.T[u],), dtype=np.int32)
        self._check(self._lib.pcl_batch_mbr(self._b, ptr(r), float(kappa), int(group)))

    def mbr_get(self, want=('logp', 'c_avg', 'lgamma', 'g')):
        """The last mbr()'s results (pcl_batch_mbr_get) as a dict: logp (U,), c_avg (U,), lgamma and g lists of (N_u, T_u) arrays; g is signed."""
        out = dict(logp=np.empty(self.U) if 'logp' in want else None, c_avg=np.empty(self.U) if 'c_avg' in want else None,
                   lgamma=np.empty(int(self._nt_off[-1])) if 'lgamma' in want else None, g=np.empty(int(self._nt_off[-1])) if 'g' in want else None)
        self._check(self._lib.pcl_batch_mbr_get(self._b, ptr(out['logp']), ptr(out['c_avg']), ptr(out['lgamma']), ptr(out['g'])))
        for k in ('lgamma', 'g'):
            if out[k] is not None:
                out[k] = [out[k][self._nt_off[u]:self._nt_off[u + 1]].reshape(self.N[u], self.T[u]) for u in range(self.U)]
        return {k: v for k, v in out.items() if v is not None}

    def mbr_posteriors(self, which):
        """The last mbr()'s posteriors into the batch, where accumulate() reads them (pcl_batch_mbr_posteriors): which = 0: ln gamma under
        kappa; +1: ln max(g, 0), the positive set of an sMBR iteration; -1: ln max(-g, 0), its negative set."""
        self._check(self._lib.pcl_batch_mbr_posteriors(self._b, int(which)))

    def ref_states(self):
        """The Viterbi alignment as mbr() takes it: per utterance the (T_u,) int32 state ids row_state[path[t]], -1 where the path sits in
        an entry or exit row.  Host NumPy on get('path') and row_states(); viterbi() must have run."""
        return [np.where(rs[p] >= 0, rs[p], -1).astype(np.int32) for rs, p in zip(self.row_states(), self.get('path'))]

    def accumulate(self, precision=PCL_F32):
        self._check(self._lib.pcl_batch_accumulate(self._b, int(precision)))

    def accumulate_exchange(self, precision=PCL_F32, c_covariance=1e-3, payload=PCL_F64, update_transitions=False, n_chunks=8):
        """The last accumulate pass of an E-step and the exchange in one pipelined call (pcl_batch_accumulate_exchange): state
        chunks leave for reduce-scatter -> M-step -> all-gather -> derive as soon as the pass is done with them.
        payload as in Engine.em_exchange (float64 unless the caller opts in to the f32 wire)."""
        self._check(self._lib.pcl_batch_accumulate_exchange(self._b, int(precision), float(c_covariance), int(payload),
                                                             1 if update_transitions else 0, int(n_chunks)))
        self.eng._model_key = None

    def accumulate_fmllr(self, utt_speaker):
        """fMLLR statistics of this batch's utterances into the engine's per-speaker sums (pcl_batch_accumulate_fmllr): utt_speaker (U,)
        int32 in [0, S) of the last Engine.fmllr_zero(S), -1 = leave the utterance out.  Needs score() and forward_backward() (or
        set_posteriors)."""
        spk = as_c(utt_speaker, np.int32).reshape(-1)
        if spk.shape != (self.U,):
            raise ValueError('utt_speaker must hold one speaker per utterance (U = %d), got %s' % (self.U, spk.shape))
        self._check(self._lib.pcl_batch_accumulate_fmllr(self._b, ptr(spk)))

    def accumulate_mllt(self, utt_keep=None):
        """The frame side of the MLLT statistics from this batch's posteriors into the sums of the last Engine.mllt_zero
        (pcl_batch_accumulate_mllt): utt_keep (U,), 0 = leave the utterance out, None = all.  Needs score() and forward_backward() (or
        set_posteriors); run accumulate() on the same batch -- the estimate takes the mixture side from the E-step statistics."""
        uk = None
        if utt_keep is not None:
            uk = as_c(np.asarray(utt_keep) != 0, np.int32).reshape(-1)
            if uk.shape != (self.U,):
                raise ValueError('utt_keep must hold one entry per utterance (U = %d), got %s' % (self.U, uk.shape))
        self._check(self._lib.pcl_batch_accumulate_mllt(self._b, ptr(uk)))

    def accumulate_lda(self, state_class=None):
        """LDA class statistics from this batch's Viterbi paths (pcl_batch_accumulate_lda) into the sums of the last Engine.lda_zero: every
        frame of an utterance align_segments() would keep counts for the class of its owner state -- state_class (J,) int32 in
        [-1, n_classes), -1 = skip; None = every state its own class.  Label-built batches only; needs score() and viterbi().  The owner
        map stays on the device."""
        sc = None
        if state_class is not None:
            sc = as_c(state_class, np.int32).reshape(-1)
            if sc.shape != (int(self.eng.J),):
                raise ValueError('state_class must hold one class per model state (J = %d), got %s' % (self.eng.J, sc.shape))
        self._check(self._lib.pcl_batch_accumulate_lda(self._b, ptr(sc)))

    def accumulate_tree(self, label_event):
        """Decision-tree context statistics from this batch's Viterbi paths (pcl_batch_accumulate_tree) into the sums of the last
        Engine.tree_zero: a frame at label position i, slice k (align_segments' slices and drop rule) counts for row
        label_event[i] * P + k; label_event (sum of the label lengths,) int32, -1 = skip the position's frames
        (ContextTree.triphone_events makes it).  Label-built batches only; needs score() and viterbi().  The owner map stays on the device."""
        le = as_c(label_event, np.int32).reshape(-1)
        labels = getattr(self, 'labels', None)        # (a host-built batch has none: the library refuses it)
        if labels is not None and le.shape != labels.shape:
            raise ValueError('label_event must hold one event per label position (%d), got %s' % (labels.size, le.shape))
        self._check(self._lib.pcl_batch_accumulate_tree(self._b, ptr(le)))

    def accumulate_hmm(self):
        """Per-unit ksai_acc / gamma_acc of every label position (LHMM.update_acc + add_acc); label-built batches only."""
        self._check(self._lib.pcl_batch_accumulate_hmm(self._b))

    def decode(self, beam=0.85, min_distinct=8, candidate=5, max_tokens=4096, lm=False, tied=False, lattice=False, max_arcs=None):
        """Token passing over the loaded pronunciation tree (Decoder.py:91-167, 250-288) for every utterance of an all-state
        batch.  Returns a list (one dict per utterance): final = [(node, score, hist)] best first, history = [(prev, node)],
        n_tokens (T,) live tokens after every frame, overflow.  lm=True: with the loaded language model at word ends
        (Engine.load_language_model); history entries are then (prev, node, chosen word id).  tied=True: the emission rows are the
        tied states Engine.tie_lexicon kept for the tree (pcl_batch_decode_tied): the model and the batch's rows are the tying's J_t states.
        lattice=True: the same results, bit for bit, and beside them the word lattice (pcl_batch_decode_lattice): at most max_arcs word-end
        records per utterance (default 128 per frame of the longest utterance) for lattice() and lattice_posteriors()."""
        self.decode_launch(beam, min_distinct, candidate, max_tokens, lm, tied, lattice, max_arcs)
        return self.decode_results()

    def decode_launch(self, beam=0.85, min_distinct=8, candidate=5, max_tokens=4096, lm=False, tied=False, lattice=False, max_arcs=None):
        """Queue the token passing (on the library's second stream, behind this batch's scoring) and return at once."""
        e = self.eng.S - 2
        lp = np.log(np.array([1.0 / (e + 2), 1.0 / (2 * e + 2)]))               # np.log(np.ones(N) / N), AcousticModel.py:1005
        args = (self._b, float(beam), int(min_distinct), int(candidate), int(max_tokens), float(lp[0]), float(lp[1]))
        self._lat = None
        if lattice:
            max_arcs = 128 * int(self.T.max()) if max_arcs is None else int(max_arcs)
            self._check(self._lib.pcl_batch_decode_lattice(*(args + (1 if lm else 0, 1 if tied else 0, max_arcs))))
            self._lat = (max_arcs, int(candidate), bool(lm))
        elif tied:
            self._check(self._lib.pcl_batch_decode_tied(*(args + (1 if lm else 0,))))
        else:
            self._check((self._lib.pcl_batch_decode_lm if lm else self._lib.pcl_batch_decode)(*args))
        self._dec_candidate, self._dec_lm = int(candidate), bool(lm)

    def decode_fetch(self):
        """Wait for the queued token passing of THIS batch (nothing else) and bring its result arrays to the host."""
        U, c, tm = self.U, self._dec_candidate, int(self.T.max())
        # page-locked result buffers: a device-to-host copy into pageable memory is staged by the runtime and was seen to return only
        # when the scoring kernel of the NEXT chunk had finished (59 ms per fetch instead of 37).  They belong to the ENGINE, one
        # grow-only set: the call below is synchronous and the arrays are copied out before it returns, so every batch can share them
        # (a ragged stream makes a new batch per chunk: per-batch buffers grew without bound and put 9 hipHostMalloc on every chunk)
        shapes = [((U,), np.int32), ((U, c), np.int32), ((U, c), np.float64), ((U, c), np.int32), ((U,), np.int32),
                  ((U, tm), np.int32), ((U, tm), np.int32), ((U, tm), np.int32), ((U,), np.int32)]
        nf, node, score, hist, hn, hp, hnode, nt, ov = self.eng._pinned_views('decode_results', shapes)
        self._check(self._lib.pcl_batch_decode_get(self._b, ptr(nf), ptr(node), ptr(score), ptr(hist), ptr(hn), ptr(hp), ptr(hnode), ptr(nt), ptr(ov)))
        raw = tuple(x.copy() for x in (nf, node, score, hist, hn, hp, hnode, nt, ov)) + (self.T.copy(),)
        if getattr(self, '_dec_lm', False):                                     # the chosen words travel behind T: an eleventh array
            hw = np.empty((U, tm), dtype=np.int32)
            self._check(self._lib.pcl_batch_decode_get_words(self._b, ptr(hw)))
            raw += (hw,)
        return raw

    @staticmethod
    def decode_unpack(raw):
        """decode_fetch's arrays as the per-utterance dicts decode() returns (host work only)."""
        nf, node, score, hist, hn, hp, hnode, nt, ov, T = raw[:10]
        out = []
        for u in range(len(nf)):
            cols = (hp[u, :hn[u]].tolist(), hnode[u, :hn[u]].tolist()) + ((raw[10][u, :hn[u]].tolist(),) if len(raw) > 10 else ())
            out.append(dict(final=list(zip(node[u, :nf[u]].tolist(), score[u, :nf[u]].tolist(), hist[u, :nf[u]].tolist())),
                            history=list(zip(*cols)),
                            n_tokens=nt[u, :T[u]].copy(), overflow=bool(ov[u])))
        return out

    def decode_results(self):
        return self.decode_unpack(self.decode_fetch())

    # ------------------------------------------------------------------ the word lattice of the last decode(lattice=True)
    def lattice_fetch(self):
        """pcl_batch_lattice_get's arrays as a dict (canonical order; arc arrays (U, max_arcs + candidate), hist_* (U, Tmax))."""
        if getattr(self, '_lat', None) is None:
            raise RuntimeError('no lattice: decode(lattice=True) first')
        max_arcs, cand, _ = self._lat
        U, A, tm = self.U, max_arcs + cand, int(self.T.max())
        i32, f64 = np.int32, np.float64
        out = dict(n_arcs=np.zeros(U, i32), n_arcs_wanted=np.zeros(U, i32), overflow=np.zeros(U, i32), frame=np.zeros((U, A), i32),
                   tok=np.zeros((U, A), i32), node=np.zeros((U, A), i32), hist=np.zeros((U, A), i32), score=np.zeros((U, A), f64),
                   term=np.zeros((U, A), f64), word=np.zeros((U, A), i32), start=np.zeros((U, A), i32), end=np.zeros((U, A), i32),
                   hist_frame=np.zeros((U, tm), i32), hist_seed=np.zeros((U, tm), f64))
        self._check(self._lib.pcl_batch_lattice_get(self._b, *[ptr(out[k]) for k in (
            'n_arcs', 'n_arcs_wanted', 'overflow', 'frame', 'tok', 'node', 'hist', 'score', 'term', 'word', 'start', 'end', 'hist_frame', 'hist_seed')]))
        return out

    def lattice(self):
        """The word lattice of every utterance, a list of Lattice objects: the arcs in canonical order (ascending (frame, tok), the closing
        arcs -- word -1 -- last), start / end node per arc (0 = START, entry k = node k + 1, END = n_entries + 1), span = (first, last)
        frame per arc, hist_frame / hist_seed per entry, n_arcs_wanted and overflow."""
        raw = self.lattice_fetch()
        out = []
        for u in range(self.U):
            n = int(raw['n_arcs'][u])
            nf = np.concatenate([[-1], raw['hist_frame'][u]]).astype(np.int64)
            lat = Lattice()
            for k in ('frame', 'tok', 'node', 'hist', 'score', 'term', 'word', 'start', 'end'):
                setattr(lat, k, raw[k][u, :n].copy())
            lat.n_entries = int((raw['hist_frame'][u] >= 0).sum())               # (the rows are cleared to -1 before every decode)
            lat.hist_frame = raw['hist_frame'][u, :lat.n_entries].copy()
            lat.hist_seed = raw['hist_seed'][u, :lat.n_entries].copy()
            lat.span = np.stack([nf[lat.start] + 1, lat.frame.astype(np.int64)], axis=1) if n else np.zeros((0, 2), np.int64)
            lat.n_arcs_wanted, lat.overflow = int(raw['n_arcs_wanted'][u]), bool(raw['overflow'][u])
            out.append(lat)
        return out

    def lattice_posteriors(self, kappa=1.0):
        """Forward-backward and Viterbi over the lattice under the acoustic scale kappa (pcl_batch_lattice_posteriors / _results; the rule:
        include/poccala_hip.h).  Per utterance a dict: lnZ, lnpost (per arc of lattice()'s order), status (0 = fine), best_score, best_arcs,
        and best = [(word id after a decode with lm -- else the node --, first frame, last frame, confidence)], the pending word of the
        closing arc last, as (node, ...)."""
        self._check(self._lib.pcl_batch_lattice_posteriors(self._b, float(kappa)))
        max_arcs, cand, lm = self._lat
        U, A, nn = self.U, max_arcs + cand, int(self.T.max()) + 3
        lnz, lnp, bn = np.zeros(U), np.zeros((U, A)), np.zeros(U, np.int32)
        ba, bs, bc, st = np.zeros((U, nn), np.int32), np.zeros(U), np.zeros((U, nn)), np.zeros(U, np.int32)
        self._check(self._lib.pcl_batch_lattice_results(self._b, ptr(lnz), ptr(lnp), ptr(bn), ptr(ba), ptr(bs), ptr(bc), ptr(st)))
        out = []
        for u, lat in enumerate(self.lattice()):
            arcs = ba[u, :bn[u]].copy()
            best = [(int(lat.word[a]) if lm and lat.word[a] >= 0 else int(lat.node[a]), int(lat.span[a, 0]), int(lat.span[a, 1]), float(c))
                    for a, c in zip(arcs, bc[u, :bn[u]])]
            out.append(dict(lnZ=float(lnz[u]), lnpost=lnp[u, :len(lat.frame)].copy(), status=int(st[u]), best_score=float(bs[u]), best_arcs=arcs, best=best))
        return out

    def refresh_transitions(self):
        """Take the engine's CURRENT unit transitions (after mstep_transitions / em_exchange); label-built batches only."""
        self._check(self._lib.pcl_batch_refresh_transitions(self._b))

    # ------------------------------------------------------------------ results on their way to the host while the GPU goes on
    def _result_shapes(self):
        """name -> (elements, dtype) of fetch_async's destinations for THIS batch (pcl_batch_sizes)."""
        nnz = np.zeros(1, dtype=np.int64)            # (label-built batches: the library built the transition lists)
        self._check(self._lib.pcl_batch_sizes(self._b, None, None, None, ptr(nnz)))
        return dict(logp=(self.U, np.float64), lgamma=(int(self._nt_off[-1]), np.float64), ksai_nz=(int(nnz[0]), np.float64),
                    path=(int(self._t_off[-1]), np.int32), point=(self.U, np.float64))

    def result_buffers(self, want=('logp', 'lgamma', 'ksai_nz', 'path', 'point'), slot=0):
        """Page-locked destination arrays for fetch_async.  They belong to the ENGINE, one grow-only set per `slot` (a pipeline that
        keeps k result sets in flight uses slots 0 .. k-1): calling this once per batch of a stream re-uses the slot's memory
        instead of page-locking ~150 MB per call until the engine closes.  ALIASING: every batch that asks for the same slot gets
        views of the SAME memory -- two batches with results in flight at once need two slots.  Asking for a slot while another
        live batch still has un-waited copies into it raises instead of handing out memory a DMA is writing."""
        busy = self.eng._slot_busy.get(slot)
        other = busy() if busy is not None else None
        if other is not None and other is not self and getattr(other, '_b', None) and other._fetch_slots:
            raise RuntimeError('result_buffers: slot %d still receives the results of another batch (fetch_wait() it first, or use another slot)' % slot)
        shapes = self._result_shapes()
        names = [k for k in ('logp', 'lgamma', 'ksai_nz', 'path', 'point') if k in want]
        views = self.eng._pinned_views('fetch_results_%d' % slot, [((shapes[k][0],), shapes[k][1]) for k in names])
        return dict(zip(names, views))

    def fetch_async(self, bufs):
        """Queue the device-to-host copies of the results named in `bufs` (result_buffers()) behind everything this batch has
        queued; returns at once.  fetch_wait() blocks until they have landed; the next compute call on this batch waits for them
        on the device.  Every buffer is checked against this batch's sizes first: a stale or short buffer would otherwise be a
        host-memory overrun written by an asynchronous DMA."""
        shapes = self._result_shapes()
        for k, a in bufs.items():
            if k not in shapes:
                raise KeyError('fetch_async: unknown result %r' % (k,))
            n, dt = shapes[k]
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.size != n or not a.flags['C_CONTIGUOUS']:
                raise ValueError('fetch_async: %s must be a C-contiguous %s array of %d elements (got %s %s)'
                                 % (k, np.dtype(dt).name, n, getattr(a, 'dtype', type(a)), getattr(a, 'shape', '')))
        g = lambda k: ptr(bufs[k]) if k in bufs else None
        self._check(self._lib.pcl_batch_fetch_async(self._b, g('logp'), g('lgamma'), g('ksai_nz'), g('path'), g('point')))
        for slot in self.eng._slots_of(bufs.values()):          # (engine-owned destinations: the slot is busy until fetch_wait)
            self.eng._slot_busy[slot] = weakref.ref(self)
            self._fetch_slots.add(slot)

    def fetch_wait(self):
        self._check(self._lib.pcl_batch_fetch_wait(self._b))
        self._fetch_slots.clear()

    def lgamma_views(self, flat):
        """fetch_async's time-major ln gamma_t(j) as the reference's (N, T) matrices (transposed views, no copy)."""
        return [flat[self._nt_off[u]:self._nt_off[u + 1]].reshape(self.T[u], self.N[u]).T for u in range(self.U)]

    # ------------------------------------------------------------------ outputs
    def regroup(self, row_unit, gmm_num):
        """Per-frame regrouping after viterbi() (AcousticModel.py:758-764 + __get_gmmdata :629-644): row_unit[u] = (N_u,)
        unit id of every HMM row.  Returns (frame_unit, frame_k): per utterance (T_u,) int32 arrays, the unit the path
        is in and the GMM state (slice of the unit's run) each frame is given to."""
        ru = self._ragged(row_unit, lambda u: (self.N[u],), dtype=np.int32)
        fu = np.empty(int(self._t_off[-1]), dtype=np.int32)
        fk = np.empty(int(self._t_off[-1]), dtype=np.int32)
        self._check(self._lib.pcl_batch_regroup(self._b, ptr(ru), int(gmm_num), ptr(fu), ptr(fk)))
        cut = lambda flat: [flat[self._t_off[u]:self._t_off[u + 1]] for u in range(self.U)]
        return cut(fu), cut(fk)

    def segments(self, row_unit, gmm_num, dropped=(), regrouped=None):
        """regroup() handed on to segmental training without the frames leaving the device: the owner state of every frame is
        frame_unit * gmm_num + frame_k (unit i owns the states i*gmm_num ..), -1 for the frames of the utterances in `dropped`
        and for the rows of the frame matrix that belong to no utterance of this batch.  `regrouped` = (frame_unit, frame_k) of an
        earlier regroup() call saves a second one.  A batch created without frame_begin has its utterances back to back from row 0."""
        fu, fk = regrouped if regrouped is not None else self.regroup(row_unit, gmm_num)
        begin = self._frame_begin if self._frame_begin is not None else self._t_off[:-1]
        state = np.full(self.eng.F, -1, dtype=np.int32)
        drop = set(int(u) for u in dropped)
        for u in range(self.U):
            if u not in drop:
                state[begin[u]:begin[u] + self.T[u]] = frame_state_of(fu[u], fk[u], gmm_num)
        return Segments(self.eng, state, self.eng.J)

    def align_segments(self, want_map=False):
        """viterbi() handed on to segmental training on the device, for a label-built batch (multi_process_data(init=False),
        AcousticModel.py:736-764): the row -> unit map comes from the batch's labels, runs and slices are regroup()'s, an utterance
        whose path misses a label unit is dropped (:751-757), and the Segments are built from the owner map without it leaving the
        device.  Returns (Segments, dropped) with dropped the sorted list of dropped utterance indices; want_map=True:
        (Segments, dropped, frame_state (F,) int32), the map segments() would have uploaded."""
        state = np.empty(max(self.eng.F, 1), dtype=np.int32) if want_map else None
        flags = np.empty(self.U, dtype=np.int32)
        h = C.c_void_p()
        self._check(self._lib.pcl_batch_align_segments(self._b, ptr(state), ptr(flags), C.byref(h)))
        seg = Segments(self.eng, None, self.eng.J, handle=h)
        dropped = np.flatnonzero(flags).tolist()
        return (seg, dropped, state[:self.eng.F]) if want_map else (seg, dropped)

    def row_states(self):
        """The row -> GMM state map as the device holds it (pcl_batch_get_states): one (N_u,) int32 array per utterance, entry and exit
        rows PCL_ROW_ENTRY / PCL_ROW_EXIT."""
        flat = np.empty(int(self._n_off[-1]), dtype=np.int32)
        self._check(self._lib.pcl_batch_get_states(self._b, ptr(flat), None))
        return [flat[self._n_off[u]:self._n_off[u + 1]] for u in range(self.U)]

    def pos_states(self):
        """A tied batch's (L_u, P) tied states per utterance: what the walks of the resident tying gave every label position."""
        P = int(self.eng.S) - 2
        flat = np.empty(int(self.labels.size) * P, dtype=np.int32)
        self._check(self._lib.pcl_batch_get_states(self._b, None, ptr(flat)))
        off = np.concatenate([[0], np.cumsum(self.label_len)]) * P
        return [flat[off[u]:off[u + 1]].reshape(-1, P) for u in range(self.U)]

    def get(self, what):
        """List of per-utterance arrays (or a (U,...) array for per-utterance scalars)."""
        code = GET[what]
        if what in ('B', 'alpha', 'beta', 'lgamma'):
            flat = np.empty(int(self._nt_off[-1]))
            self._check(self._lib.pcl_batch_get(self._b, code, ptr(flat)))
            return [flat[self._nt_off[u]:self._nt_off[u + 1]].reshape(self.N[u], self.T[u]) for u in range(self.U)]
        if what == 'ksai':
            flat = np.empty(int(self._nn_off[-1]))
            self._check(self._lib.pcl_batch_get(self._b, code, ptr(flat)))
            return [flat[self._nn_off[u]:self._nn_off[u + 1]].reshape(self.N[u], self.N[u]) for u in range(self.U)]
        if what == 'ksai_nz':
            if self._nnz_off is None:
                raise RuntimeError('set_transitions first')
            flat = np.empty(int(self._nnz_off[-1]))
            self._check(self._lib.pcl_batch_get(self._b, code, ptr(flat)))
            return [flat[self._nnz_off[u]:self._nnz_off[u + 1]] for u in range(self.U)]
        if what in ('gamma', 'pi'):
            flat = np.empty(int(self._n_off[-1]))
            self._check(self._lib.pcl_batch_get(self._b, code, ptr(flat)))
            return [flat[self._n_off[u]:self._n_off[u + 1]] for u in range(self.U)]
        if what == 'path':
            flat = np.empty(int(self._t_off[-1]), dtype=np.int32)
            self._check(self._lib.pcl_batch_get(self._b, code, ptr(flat)))
            return [flat[self._t_off[u]:self._t_off[u + 1]] for u in range(self.U)]
        if what in ('logp', 'point'):
            out = np.empty(self.U)
        elif what == 'npass':
            out = np.empty(self.U, dtype=np.int32)
        elif what == 'qtrace':
            out = np.empty((self.U, PCL_MAX_PASS))
        else:
            raise KeyError(what)
        self._check(self._lib.pcl_batch_get(self._b, code, ptr(out)))
        return out


def frame_state_of(frame_unit, frame_k, gmm_num):
    """The two arrays pcl_batch_regroup writes -> the owner GMM state of every frame (-1 where either is negative)."""
    fu, fk = np.asarray(frame_unit, dtype=np.int64), np.asarray(frame_k, dtype=np.int64)
    return np.where((fu >= 0) & (fk >= 0), fu * int(gmm_num) + fk, -1).astype(np.int32)


class Segments(object):
    """The frames of every GMM state, on the device, for training scheme 1 (AcousticModel.__cal_gmm, AcousticModel.py:532-561):
    `kmeans` then `em` make the engine's model from them, all states at once.  States with fewer frames than mixtures are left
    untouched and reported as -1, as the reference skips them (:549-551)."""

    def __init__(self, engine, frame_state, J, handle=None):
        self.eng = engine
        self._lib = engine._lib
        self.J = int(J)
        if handle is not None:                        # a pcl_seg the library built itself (Engine.uniform_segments, Batch.align_segments)
            self._s = handle
        else:
            self._s = C.c_void_p()
            st = as_c(frame_state, np.int32).reshape(-1)
            engine._check(self._lib.pcl_seg_create(engine._ctx, st.shape[0], self.J, ptr(st), C.byref(self._s)))
        engine._segments.add(self)
        self.counts = self._get('counts', self.J)
        self.K = 0
        self.D = engine.FD

    def _get(self, what, n):
        out = np.empty(n, dtype=np.int32)
        self.eng._check(self._lib.pcl_seg_get(self._s, SEG_GET[what], ptr(out)))
        return out

    @property
    def order(self):
        """Frame rows of state 0, then state 1, ...: each in ascending row order."""
        return self._get('order', int(self.counts.sum()))

    def split(self, flat):
        """A (sum n_j, ...) array in segment order as a list of per-state arrays."""
        off = np.concatenate([[0], np.cumsum(self.counts)])
        return [flat[off[j]:off[j + 1]] for j in range(self.J)]

    def kmeans(self, K, seed=0, max_sweeps=100, precision=PCL_F32, init_centres=None):
        """k-means++ seeding (or init_centres (J,K,D)) + Lloyd sweeps per state, then the engine's model becomes (J,K,D): cluster
        means, floored mean squared deviations, n_jk / n_j.  NOT the reference routine's arithmetic (include/poccala_hip.h,
        pcl_seg_kmeans): textbook k-means++ / Lloyd, deterministic for a seed.  Returns sweeps per state (-1: skipped)."""
        sweeps = np.empty(self.J, dtype=np.int32)
        ic = None
        if init_centres is not None:
            ic = as_c(init_centres, np.float64)
            if ic.ndim != 3 or ic.shape[:2] != (self.J, int(K)):
                raise ValueError('init_centres must be (J, K, D), got %s' % (ic.shape,))
        self.eng._check(self._lib.pcl_seg_kmeans(self._s, int(K), int(seed) & ((1 << 64) - 1), int(max_sweeps), int(precision), ptr(ic), ptr(sweeps)))
        self.K = int(K)
        self.eng.J, self.eng.M, self.eng.D = self.J, int(K), self.D
        self.eng._model_key = None
        return sweeps

    def assignments(self):
        return self._get('assign', int(self.counts.sum()))

    def seed_positions(self):
        return self._get('seeds', self.J * self.K).reshape(self.J, self.K)

    def centres(self):
        out = np.empty((self.J, self.K, self.D))
        self.eng._check(self._lib.pcl_seg_centres(self._s, ptr(out)))
        return out

    def em(self, c_covariance=1e-3, q_threshold=1.28, max_iters=100, precision=PCL_F32, trace=False):
        """Clustering.GMM.em (Clustering.py:695-719, smem=False) for every state at once from the engine's model.  Returns
        (iters, q): loop bodies run per state (-1: skipped, fewer frames than mixtures) and the last accepted Q; with trace=True also
        the (J, max_iters) Q of every loop body (NaN beyond)."""
        iters = np.empty(self.J, dtype=np.int32)
        q = np.empty(self.J)
        qt = np.empty((self.J, int(max_iters))) if trace else None
        self.eng._check(self._lib.pcl_seg_em(self._s, float(c_covariance), float(q_threshold), int(max_iters), int(precision), ptr(iters), ptr(q), ptr(qt)))
        self.eng._model_key = None
        return (iters, q, qt) if trace else (iters, q)

    def close(self):
        if getattr(self, '_s', None):
            if getattr(self.eng, '_ctx', None):
                self._lib.pcl_seg_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------- sentence HMM construction
def embedded_structure(n_units, unit_trans, s=5):
    """Host part of AcousticModel.embedded (AcousticModel/AcousticModel.py:957-1014) for one label:
    the (N,N) transition matrix and the uniform 1/N pi.  unit_trans: list of (S,S) matrices, one
    per label position.  The emission rows are laid out by `embedded_row_states`."""
    e = s - 2
    n = e * n_units + 2
    a = np.zeros((n, n))
    a[:s - 1, :s] = unit_trans[0][:-1]
    for i in range(n_units):
        lo = i * e + 1
        a[lo:lo + e, lo - 1:lo - 1 + s] = unit_trans[i][1:-1]
    pi = np.ones(n) / n
    return a, pi


def loop_structure(unit_trans, unit_prior=None, s=5):
    """The (N,N) transition matrix and uniform pi of a unit loop over the whole inventory, N = (s-2) len(unit_trans) + 2 (Engine.loop_batch):
    row 0 the entry, unit i's emitting rows 1 + i (s-2) ..., the last row the exit.  Inside its own block a row keeps unit_trans[i][1:-1];
    what it sends to the unit's exit column goes to the first emitting row of every unit, times unit_prior (normalised; default uniform);
    the entry row goes to those rows with unit_prior; the exit row has no successor."""
    e, n_units = s - 2, len(unit_trans)
    prior = np.ones(n_units) if unit_prior is None else np.asarray(unit_prior, dtype=np.float64).reshape(-1)
    if prior.shape != (n_units,) or not (np.all(prior >= 0) and prior.sum() > 0):
        raise ValueError('unit_prior must hold one weight >= 0 per unit, not all of them 0')
    prior = prior / prior.sum()
    n = e * n_units + 2
    first = 1 + e * np.arange(n_units)
    a = np.zeros((n, n))
    a[0, first] = prior
    for i in range(n_units):
        t = np.asarray(unit_trans[i], dtype=np.float64)
        lo = 1 + i * e
        a[lo:lo + e, lo:lo + e] = t[1:-1, 1:-1]
        a[lo:lo + e, first] += t[1:-1, -1][:, None] * prior[None, :]
    return a, np.ones(n) / n


def embedded_row_states(unit_state_ids, s=5):
    """Row -> GMM state id map of the sentence HMM: entry row, each unit's S-2 emitting states,
    exit row (AcousticModel.py:990-1001).  unit_state_ids: (L, S-2) global GMM state ids."""
    ids = np.asarray(unit_state_ids, dtype=np.int32).reshape(-1)
    return np.concatenate([[PCL_ROW_ENTRY], ids, [PCL_ROW_EXIT]]).astype(np.int32)


def make_sentence_batch(engine, unit_ids, T, frame_begin, unit_trans, s=5, unit_state_ids=None):
    """Build the batch for a list of labels.  unit_ids[u]: sequence of unit indices (label of
    utterance u); unit i owns GMM states i*(S-2) .. i*(S-2)+S-3 of the uploaded model and the
    transition matrix unit_trans[i] (S,S).  unit_state_ids[u]: the (L_u, S-2) GMM state ids of the
    label's emitting rows in place of unit*(S-2) + k -- tied states (ContextTree.Tree.unit_state_ids).
    Returns (batch, N)."""
    e = s - 2
    n = np.array([e * len(l) + 2 for l in unit_ids], dtype=np.int32)
    if unit_state_ids is not None and len(unit_state_ids) != len(unit_ids):
        raise ValueError('unit_state_ids must hold one (L, %d) array per utterance' % e)
    b = engine.batch(n, T, frame_begin)
    log_a, log_pi, rows = [], [], []
    with np.errstate(divide='ignore'):
        for u, lab in enumerate(unit_ids):
            lab = np.asarray(lab, dtype=np.int64)
            a, pi = embedded_structure(len(lab), [unit_trans[i] for i in lab], s)
            log_a.append(np.log(a))
            log_pi.append(np.log(pi))
            ids = lab[:, None] * e + np.arange(e)[None, :]
            if unit_state_ids is not None:
                ids = np.asarray(unit_state_ids[u])
                if ids.shape != (len(lab), e):
                    raise ValueError('unit_state_ids[%d] must be (%d, %d), got %s' % (u, len(lab), e, ids.shape))
            rows.append(embedded_row_states(ids, s))
    b.set_transitions(log_a, log_pi)
    b.set_states(rows)
    return b, n
