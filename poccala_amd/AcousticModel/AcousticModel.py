"""Drop-in for the hot-path part of AcousticModel/AcousticModel.py.

Mirrored (starred): `embedded` :957-1014, `viterbi` :1016-1027, `discriminate`
:937-955, `VirtualState` :1029-1043, plus `init_unit` :164-226 / `init_parameter` :228-240 so that a
per-utterance E-step or alignment can be written exactly as the reference's workers write it
(`multi_embedded_training_1` :884-916, `multi_process_data` :723-768).  Batched equivalents that keep
everything on the GPU are `estep_batch` / `align_batch`, and `train_segments_batch` / `train_segments_data` for training
scheme 1 (`__cal_gmm` :532-561: clustering + stand-alone EM of every state), and `flat_start_batch` (`__flat_start` :479-517) /
`init_segments_batch` (`multi_process_data(init=True)` :734-735) for the model-free step either scheme begins with.  `mixup_batch` grows the
units' models between rounds of EM by splitting mixtures on the device (no counterpart in the reference).  `load_audio` is `__load_audio` (:463-477: wav -> MFCC ->
VAD); `load_audio_batch` does it for many files in one call and leaves the frames resident.  Orchestration (Pool fan-out, file
walking, recording) is out of scope.
"""
import os

import numpy as np

from ..Exceptions import NullLog, UnitFileExistsError
from .._lib import PCL_F32, PCL_F64
from ..runtime import default_engine
from ..StatisticalModel.Clustering import Clustering
from ..StatisticalModel.DataInitialization import DataInitialization
from ..StatisticalModel.LHMM import LHMM


class AcousticModel(DataInitialization):
    def __init__(self, log=None, unit_type='XIF_tone', mode=0, processes=None, job_id=0, console=True, state_num=5,
                 mix_level=1, dct_num=13, delta_1=True, delta_2=True, parameters_path=None):
        super().__init__()
        self.log = log if log is not None else NullLog()
        self.__unit_type = unit_type
        self.__state_num = state_num
        self.__mix_level = mix_level
        self.__vector_size = dct_num * (3 if delta_2 else 2 if delta_1 else 1)     # AcousticModel.py:84-88
        self.__dct_num, self.__delta_1, self.__delta_2 = dct_num, delta_1, delta_2
        self.__address = parameters_path or os.environ.get('parameters_file_path', '.')
        self.__loaded_units = []
        self.processes = processes or 1
        # the two workers at batched speed (multi_embedded_training_1 / multi_process_data below): what the calls queued
        self.__queued = {'train': [], 'align': []}
        self.__queued_frames = 0
        self.__flush_registered = self.__warned_worker = False
        self.__data_files = 0
        self.flush_frames = 1 << 19            # flush by itself once this many frames are queued (bounds the host copy)
        self.worker_precision = None           # None: f32-class E-step, float64 alignment (bit-exact paths)
        self.worker_units = None               # {unit: LHMM}: unit models held in memory instead of re-read from the parameter tree
        self.worker_engine = None

    loaded_units = property(lambda self: self.__loaded_units)
    statenum = property(lambda self: self.__state_num)

    def load_audio(self, audiopath):
        """__load_audio (AcousticModel.py:463-477): the wav file's MFCC with this object's dct_num / delta_1 / delta_2 at nfft = 512,
        then the voice-activity detector's survivors, (T', D) float64."""
        from ..StatisticalModel.AudioProcessing import AudioProcessing
        mfcc = AudioProcessing.MFCC(self.__dct_num)
        mfcc.init_audio(path=audiopath)
        m = mfcc.mfcc(nfft=512, d1=self.__delta_1, d2=self.__delta_2)
        mfcc.wav.close()                                           # (the samples have been read; the reference leaves the file open)
        vad = AudioProcessing.VAD()
        vad.init_mfcc(m)
        return vad.mfcc()

    def load_audio_batch(self, paths, engine=None, fetch=True):
        """load_audio for many files through Engine.frontend: one MFCC + VAD + compaction on the device, the survivors left resident as
        the engine's frame matrix.  Returns (lens, begin, data_list): data_list[u] = what load_audio(paths[u]) returns (fetch=False:
        None, nothing comes back to the host); an utterance that kept no frame has lens[u] = 0 and a (0, D) entry, which estep_batch /
        align_batch / segment_batch / regroup_batch / train_segments_batch skip.  Those helpers take data_list and upload it again: the
        route WITHOUT a feature upload is engine.label_batch / all_state_batch on (lens, begin) of the non-empty utterances, as
        INTEGRATION.md shows.  The files must share one sampling rate.  init_audio reads the samples as np.int16 and they are handed on
        as they are: the call takes Engine.frontend's int16 route (int16 on the wire, converted in the MFCC kernel), same bits."""
        from ..StatisticalModel.AudioProcessing import AudioProcessing
        eng = engine or default_engine()
        sigs, rate = [], None
        for p in paths:
            m = AudioProcessing.MFCC(self.__dct_num)
            m.init_audio(path=p)
            if rate is not None and m.params[2] != rate:
                raise ValueError('load_audio_batch: %s is sampled at %d Hz, the files before it at %d' % (p, m.params[2], rate))
            rate = m.params[2]
            sigs.append(m.data)
            m.wav.close()
        d2 = bool(self.__delta_1 and self.__delta_2)               # MFCC.mfcc computes the second deltas only inside d1 (:440-447)
        res = eng.frontend(sigs, rate, vec_num=self.__dct_num, nfft=512, d1=bool(self.__delta_1), d2=d2, fetch=fetch)
        if not fetch:
            return res[0], res[1], None
        lens, begin, rows = res
        return lens, begin, [rows[b:b + n] for b, n in zip(begin, lens)]

    def load_unit(self, unit_type=None, unit_file=None):
        """AcousticModel.load_unit (AcousticModel.py:134-161): the inventory is the file `$unit_file_path/<unit_type>` (unit_type given:
        it becomes the model's unit type); a missing file raises UnitFileExistsError; the parameter tree `<parameters path>/<unit_type>`
        is created.  Line 1 of the file is a description, the rest comma-separated units.  `unit_file=` (keyword, not in the
        reference) reads a file by its path instead and creates nothing."""
        if unit_file is None:
            if unit_type:
                self.__unit_type = unit_type
            base = os.environ.get('unit_file_path')
            if base is None:
                raise KeyError('unit_file_path')             # (the reference reads os.environ['unit_file_path'] at import, AcousticModel.py:25)
            unit_file = os.path.abspath(base) + '/' + self.__unit_type
            if not os.path.exists(unit_file):
                raise UnitFileExistsError(self.__unit_type, self.log)
            os.makedirs(os.path.join(self.__address, self.__unit_type), exist_ok=True)
        with open(unit_file) as f:
            f.readline()
            for line in f:
                self.__loaded_units.extend(u for u in line.strip('\n').split(',') if u)

    # ------------------------------------------------------------------ unit HMMs
    def init_unit(self, unit, new_log=True, fix_code=0):
        """5-state left-right unit HMM: entry / S-2 GMM states / exit, flat-start transitions
        (AcousticModel.py:164-226)."""
        s = self.__state_num
        states = {i: unit for i in range(s)}
        transmat = np.zeros((s, s))
        transmat[0][1] = 1.
        for j in range(1, s - 1):
            transmat[j][j] = 0.5
            transmat[j][j + 1] = 0.5
        gmm = [Clustering.GMM(self.log, dimension=self.__vector_size, mix_level=self.__mix_level, gmm_id=k)
               for k in range(s - 2)]
        prof = [AcousticModel.VirtualState(1.)] + gmm + [AcousticModel.VirtualState(0.)]
        return LHMM(states, s, self.log, transmat=transmat, profunc=prof, fix_code=fix_code)

    def unit_path(self, unit):
        return '%s/%s/%s' % (self.__address, self.__unit_type, unit)

    def init_parameter(self, unit, hmm):
        hmm.init_parameter(self.unit_path(unit))
        for i in range(1, self.__state_num - 1):
            hmm.profunction[i].init_parameter(self.unit_path(unit))

    def save_parameter(self, unit, hmm):
        os.makedirs(self.unit_path(unit), exist_ok=True)
        hmm.save_parameter(self.unit_path(unit))
        for i in range(1, self.__state_num - 1):
            hmm.profunction[i].save_parameter(self.unit_path(unit))

    def save_acc(self, unit, hmm):
        os.makedirs(self.unit_path(unit), exist_ok=True)
        hmm.save_acc(self.unit_path(unit))
        for i in range(1, self.__state_num - 1):
            hmm.profunction[i].save_acc(self.unit_path(unit))

    # ------------------------------------------------------------------ A7 embedded (AcousticModel.py:957-1014)
    def embedded(self, label, hmm_list, data_index, alter=15):
        s = self.__state_num
        e = s - 2
        n = e * len(hmm_list) + 2

        def embedded_states():
            names = [label[0]]
            for u in label:
                names.extend([u] * e)
            names.append(label[len(label) - 1])
            return dict(enumerate(names))

        def embedded_transmat():
            a = np.zeros((n, n))
            a[:s - 1, :s] = hmm_list[0].transmat[:-1]
            for i in range(len(label)):
                lo = i * e + 1
                a[lo:lo + e, lo - 1:lo - 1 + s] = hmm_list[i].transmat[1:-1]
            return a

        def embedded_prob():
            rows = [hmm_list[0].B_p[data_index][0:-1]]
            for i in range(1, len(label)):
                rows.append(hmm_list[i].B_p[data_index][1:-1, :])
            rows.append(hmm_list[len(label) - 1].B_p[data_index][-1:, :])
            return np.concatenate(rows, axis=0)

        def embedded_pi():
            return np.ones((n,)) / n

        funcs = [embedded_states, embedded_transmat, embedded_prob, embedded_pi]
        return [funcs[k]() for k in range(4) if 2 ** (3 - k) & alter]

    # ------------------------------------------------------------------ A14 wrappers
    def viterbi(self, complex_states, complex_transmat, complex_prob, complex_pi):
        return LHMM.viterbi(self.log, complex_states, complex_transmat, complex_prob, complex_pi, convert=True,
                            show_mark_state=True)

    @staticmethod
    def discriminate(unit, sequence):
        """Frame indices labelled `unit`, split into contiguous runs (AcousticModel.py:937-955)."""
        loc = np.where(np.asarray(sequence) == unit)[0]
        if len(loc) == 0:
            return []
        return np.split(loc, np.where(np.diff(loc) != 1)[0] + 1)

    class VirtualState(object):
        """Constant-score pdf of the non-emitting entry/exit states (AcousticModel.py:1029-1043)."""

        constant_score = True                  # point() does not look at the frame: callers may evaluate it once per utterance

        def __init__(self, p=0.):
            self.__p = p

        def point(self, x, log=False, standard=False, record=False):
            if log:
                with np.errstate(divide='ignore'):
                    return np.log(self.__p)
            return self.__p

    # ------------------------------------------------------------------ batched, GPU-resident equivalents
    def _model_arrays(self, unit_hmms):
        units = sorted(unit_hmms)
        idx = {u: i for i, u in enumerate(units)}
        arrs = [unit_hmms[u].profunction[1 + k].model_arrays() for u in units for k in range(self.__state_num - 2)]
        trans = [np.asarray(unit_hmms[u].transmat, dtype=np.float64) for u in units]
        return units, idx, (np.stack([a[0] for a in arrs]), np.stack([a[1] for a in arrs]), np.stack([a[2] for a in arrs])), trans

    @staticmethod
    def _nonempty(data_list):
        """Indices of the utterances that have frames.  The voice-activity detector may keep no frame of an utterance (load_audio /
        load_audio_batch then give a (0, D) array): the batch helpers below leave such an utterance out of the device batch -- a
        sentence HMM over zero frames has no alignment and adds nothing to any accumulator -- and keep their results aligned with
        the input lists."""
        res = AcousticModel._resident(data_list)
        keep = [u for u, d in enumerate(data_list) if len(d) > 0] if res is None else np.flatnonzero(res[0] > 0).tolist()
        if not keep:
            raise ValueError('every utterance of the batch is empty (no frame survived the voice-activity detector)')
        return keep

    @staticmethod
    def _resident(data_list):
        """The batch helpers take a list of (T_u, D) arrays, which they upload, or the (lens, begin) of frames already resident
        (Engine.frontend / load_audio_batch(fetch=False)), the form flat_start_batch accepts: (lens int32, begin int64) for the
        second form, None for the first."""
        if isinstance(data_list, tuple) and len(data_list) == 2 and np.ndim(data_list[0]) == 1:
            return np.asarray(data_list[0], dtype=np.int32), np.asarray(data_list[1], dtype=np.int64)
        return None

    @staticmethod
    def _utt_count(data_list):
        res = AcousticModel._resident(data_list)
        return len(data_list) if res is None else len(res[0])

    @staticmethod
    def _utt_subset(data_list, keep):
        res = AcousticModel._resident(data_list)
        return [data_list[u] for u in keep] if res is None else (res[0][keep], res[1][keep])

    def _sentence_batch(self, labels, data_list, unit_hmms, engine):
        units, idx, (mean, var, w), trans = self._model_arrays(unit_hmms)
        engine.load_model(mean, var, w)
        engine.load_units(np.stack(trans))
        res = self._resident(data_list)
        if res is not None:                                  # frames already resident: nothing is uploaded
            lens, begin = res
        else:
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d) for d in data_list], axis=0))
        unit_ids = [np.array([idx[u] for u in lab], dtype=np.int32) for lab in labels]
        b = engine.label_batch(unit_ids, lens, begin)        # AcousticModel.embedded for every utterance, in the library
        return b, b.N, units, idx

    def align_batch(self, labels, data_list, unit_hmms, precision=PCL_F64, engine=None):
        """Forced alignment of many utterances at once (call stack C, AcousticModel.py:723-768):
        returns [(point, unit-name sequence)] like AcousticModel.viterbi does per utterance.  An utterance without frames is
        skipped: (nan, empty sequence) in its place."""
        engine = engine or default_engine()
        keep = self._nonempty(data_list)
        if len(keep) < self._utt_count(data_list):          # an empty utterance: (nan, no names) in its place
            res = self.align_batch([labels[u] for u in keep], self._utt_subset(data_list, keep), unit_hmms, precision, engine)
            out = [(float('nan'), np.array([], dtype=str))] * self._utt_count(data_list)
            for u, r in zip(keep, res):
                out[u] = r
            return out
        b, n, units, idx = self._sentence_batch(labels, data_list, unit_hmms, engine)
        b.score(precision)
        b.viterbi()
        pts, paths = b.get('point'), b.get('path')
        b.close()
        e = self.__state_num - 2
        out = []
        for u, lab in enumerate(labels):
            names = np.array([lab[0]] + [x for x in lab for _ in range(e)] + [lab[-1]])
            out.append((float(pts[u]), names[paths[u]]))
        return out

    def estep_batch(self, labels, data_list, unit_hmms, fix_code=0, precision=PCL_F32, engine=None):
        """E-step of many utterances at once (call stack B, AcousticModel.py:884-916).  Returns
        (stats, hmm_acc, logp): `stats` = linear-domain GMM statistics per state (engine.stats_download,
        states ordered unit-major over sorted(unit_hmms)); `hmm_acc[unit]` = (ksai_acc (S-2,S),
        gamma_acc (S-2,)) log-domain, merged over every occurrence as LHMM.add_acc does (LHMM.py:149-161,
        473-500).  Everything per utterance x label position runs in the library: the sentence HMMs are built
        from the labels there (pcl_batch_create_labels) and the per-unit merge is a kernel
        (pcl_batch_accumulate_hmm); nothing here loops over utterances.  An utterance without frames is skipped (logp = nan)."""
        engine = engine or default_engine()
        keep = self._nonempty(data_list)
        if len(keep) < self._utt_count(data_list):          # empty utterances add nothing to the statistics: logp = nan in their place
            stats, hmm_acc, lp = self.estep_batch([labels[u] for u in keep], self._utt_subset(data_list, keep), unit_hmms, fix_code, precision,
                                                  engine)
            logp = np.full(self._utt_count(data_list), np.nan)
            logp[keep] = lp
            return stats, hmm_acc, logp
        b, n, units, idx = self._sentence_batch(labels, data_list, unit_hmms, engine)
        b.score(precision)
        b.forward_backward(fix_pi=bool(fix_code & 1))
        engine.stats_zero()                       # GMM statistics and the per-unit HMM accumulators
        stats = None
        if not fix_code & 2:
            b.accumulate(precision)
            stats = engine.stats_download()
        hmm_acc = {}
        if not fix_code & 4:
            b.accumulate_hmm()
            ks, ga = engine.hmm_acc_download()
            seen = np.bincount(b.labels, minlength=len(units)) > 0
            hmm_acc = {unit: (ks[i], ga[i]) for i, unit in enumerate(units) if seen[i]}
        logp = b.get('logp')
        b.close()
        return stats, hmm_acc, logp

    # ------------------------------------------------------------------ what follows the two workers in the reference
    def segment_batch(self, labels, data_list, unit_hmms, precision=PCL_F64, engine=None):
        """Alignment -> per-unit data segments for many utterances (the loop at AcousticModel.py:758-764:
        discriminate + __save_data): returns {unit: [frame blocks]} where each block is the (n,D) slice of one
        contiguous run of that unit, in utterance order; an utterance whose path misses a label unit is
        dropped, as the reference does (:754-757)."""
        out = {}
        dropped = []
        for u, (point, names) in enumerate(self.align_batch(labels, data_list, unit_hmms, precision, engine)):
            if len(set(names)) < len(set(labels[u])):
                dropped.append(u)
                continue
            data = np.asarray(data_list[u])
            for unit in set(labels[u]):
                for loc in AcousticModel.discriminate(unit, names):
                    out.setdefault(unit, []).append(data[loc])
        return out, dropped

    def eq_segment(self, data, arg=None, mode='e', save=None):
        """AcousticModel.__eq_segment (AcousticModel.py:587-627).  mode 'e': the utterance is cut into len(arg) equal
        chunks, one per label unit, handed to `save(unit, block)` (the reference's __save_data pickles them); the
        remainder frames are dropped.  mode 'g': one block cut into `arg` slices, the last takes the remainder."""
        if mode == 'e':
            chunk = len(data) // len(arg)
            for i, u in enumerate(arg):
                if save is not None:
                    save(u, data[i * chunk:(i + 1) * chunk])
            return None
        if mode == 'g':
            chunk = len(data) // arg
            out = [data[k * chunk:(k + 1) * chunk] for k in range(arg - 1)]
            out.append(data[(arg - 1) * chunk:])
            return out
        raise ValueError('eq_segment: mode must be \'e\' or \'g\'')   # the reference raises ClassError here

    def get_gmmdata(self, data):
        """AcousticModel.__get_gmmdata (AcousticModel.py:629-644): the data of each of the unit's S-2 GMM states."""
        gmm_num = self.__state_num - 2
        parts = [self.eq_segment(block, gmm_num, mode='g') for block in data]
        return [np.concatenate([p_[k] for p_ in parts], axis=0) for k in range(gmm_num)]

    def _align_regroup(self, labels, data_list, unit_hmms, precision, engine):
        """Viterbi + pcl_batch_regroup for many utterances.  Returns (batch -- still open --, units, idx, row_unit, frame_unit,
        frame_k, dropped): dropped = the utterances whose path misses a label unit (AcousticModel.py:754-757)."""
        engine = engine or default_engine()
        b, n, units, idx = self._sentence_batch(labels, data_list, unit_hmms, engine)
        b.score(precision)
        b.viterbi()
        s = self.__state_num
        row_unit = []
        for lab in labels:
            ids = np.repeat([idx[u] for u in lab], s - 2)
            row_unit.append(np.concatenate([[ids[0]], ids, [ids[-1]]]).astype(np.int32))     # entry / exit rows: first / last unit
        fu, fk = b.regroup(row_unit, s - 2)
        dropped = [u for u, lab in enumerate(labels) if len(np.unique(fu[u])) < len(set(lab))]
        return b, units, idx, row_unit, fu, fk, dropped

    def regroup_batch(self, labels, data_list, unit_hmms, precision=PCL_F64, engine=None):
        """Forced alignment -> the re-estimation data of every GMM state, for many utterances, on the device: Viterbi
        (`align_batch`'s kernels), then `pcl_batch_regroup` instead of discriminate + __save_data + __get_gmmdata
        (AcousticModel.py:758-764, 629-644).  Returns ({unit: [S-2 arrays (n_k, D)]}, dropped): for each unit the frames
        of its GMM states, in utterance then time order; an utterance whose path misses a label unit is dropped
        (:754-757)."""
        keep = self._nonempty(data_list)
        if len(keep) < len(data_list):          # empty utterances are dropped like the ones whose path misses a unit
            out, dropped = self.regroup_batch([labels[u] for u in keep], [data_list[u] for u in keep], unit_hmms, precision, engine)
            return out, sorted((set(range(len(data_list))) - set(keep)) | {keep[u] for u in dropped})
        b, units, idx, row_unit, fu, fk, dropped = self._align_regroup(labels, data_list, unit_hmms, precision, engine)
        b.close()
        s = self.__state_num
        names = {i: u for u, i in idx.items()}
        out = {}
        for u, lab in enumerate(labels):
            if u in dropped:
                continue
            data = np.asarray(data_list[u])
            for i in np.unique(fu[u]):
                slot = out.setdefault(names[i], [[] for _ in range(s - 2)])
                for k in range(s - 2):
                    slot[k].append(data[(fu[u] == i) & (fk[u] == k)])
        d = np.asarray(data_list[0]).shape[1]
        return ({unit: [np.concatenate(parts, axis=0) if parts else np.zeros((0, d)) for parts in slots]
                 for unit, slots in out.items()}, dropped)

    # ------------------------------------------------------------------ training scheme 1 (AcousticModel.training mode 1, :771-840)
    @staticmethod
    def _no_smem(smem):
        if smem:
            raise NotImplementedError('SMEM split / merge is outside the hot path (SURVEY section 2 row 3)')

    def _train_segments(self, engine, seg, units, unit_hmms, init, mix_level, smem, c_covariance, seed, precision):
        """ClusterInitialization.kmeans (when the model is new or its mixture count changes, __cal_gmm :552) + GMM.em for every
        state of every unit at once, from the engine's model; the result goes back into the units' GMM objects."""
        e = self.__state_num - 2
        k = int(mix_level) if mix_level is not None else engine.M
        try:
            if init or k != engine.M:
                seg.kmeans(k, seed=seed, precision=precision)
            iters, q = seg.em(c_covariance=c_covariance, precision=precision)
            counts = seg.counts.copy()
        finally:
            seg.close()
        mean, var, w = engine.model_download()
        out = {}
        for ui, unit in enumerate(units):
            js = slice(ui * e, (ui + 1) * e)
            for kk in range(e):
                j = ui * e + kk
                if iters[j] >= 0:                                     # a state with fewer frames than mixtures keeps its model (:549-551)
                    unit_hmms[unit].profunction[1 + kk].set_model(mean[j], var[j], w[j])
            out[unit] = (iters[js].copy(), q[js].copy(), iters[js] < 0)
        self.last_segment_counts = {unit: counts[ui * e:(ui + 1) * e] for ui, unit in enumerate(units)}
        return out

    def train_segments_batch(self, labels, data_list, unit_hmms, init=False, mix_level=None, smem=False, c_covariance=1e-3, seed=0,
                             precision=PCL_F64, engine=None):
        """Training scheme 1 for many utterances at once: forced alignment, then regrouping, the drop rule and the per-state frame
        lists in one device call (Batch.align_segments; the same result as `regroup_batch`'s route), then -- without the frames or the
        owner map leaving the device -- clustering (init=True, or mix_level differs from the model's) and the stand-alone
        EM of every GMM state of every unit in one batch of launches (AcousticModel.__cal_gmm, AcousticModel.py:532-561, for every
        unit of multi_training :771-840).  The units' GMM objects receive the new parameters.  Returns {unit: (iters (S-2,),
        q (S-2,), skipped (S-2,) bool)}; utterances whose path misses a label unit are dropped (:754-757) and listed in
        `self.last_dropped`.  `data_list` is a list of (T_u, D) arrays (uploaded here) or the (lens, begin) of frames already resident
        (Engine.frontend / load_audio_batch(fetch=False)), of which nothing is uploaded; utterances of length 0 are left out and
        listed in `last_dropped`.  The clustering is textbook k-means++ / Lloyd, not the reference routine's arithmetic
        (Clustering.ClusterInitialization)."""
        self._no_smem(smem)
        engine = engine or default_engine()
        keep = self._nonempty(data_list)
        n_utts = self._utt_count(data_list)
        if len(keep) < n_utts:                  # empty utterances are dropped like the ones whose path misses a unit
            out = self.train_segments_batch([labels[u] for u in keep], self._utt_subset(data_list, keep), unit_hmms, init, mix_level, smem,
                                            c_covariance, seed, precision, engine)
            self.last_dropped = sorted((set(range(n_utts)) - set(keep)) | {keep[u] for u in self.last_dropped})
            return out
        b, n, units, idx = self._sentence_batch(labels, data_list, unit_hmms, engine)
        try:
            b.score(precision)
            b.viterbi()
            seg, self.last_dropped = b.align_segments()      # regrouping, drop rule and owner map: one kernel, nothing per utterance here
        finally:
            b.close()
        return self._train_segments(engine, seg, units, unit_hmms, init, mix_level, smem, c_covariance, seed, precision)

    # ------------------------------------------------------------------ starting from nothing: what either scheme begins with
    def flat_start_batch(self, data, unit_hmms, proportion=0.25, step=1, differentiation=True, coefficient=1., seed=None, engine=None):
        """AcousticModel.__flat_start (AcousticModel.py:479-517) on the device.  `data` is a list of (T_u, D) arrays (uploaded here), or
        the (lens, begin) of frames already resident (Engine.frontend / load_audio_batch(fetch=False)): the global mean and variance
        of data[::step] of the first int(len * proportion) utterances, then every mixture of every GMM state of every unit in
        `unit_hmms` set to mean + diff[m] * variance / variance / weight 1 / mix_level, with ONE draw diff = (random((M, 1)) -
        random((M, 1))) * coefficient shared by all of them (differentiation=False: zero).  seed=None draws from NumPy's global
        generator as the reference does; a seed draws the same numbers np.random.seed(seed) would have given.  The model is left
        resident in the engine (states unit-major over sorted(unit_hmms), as every batch helper lays them out) AND written into
        the units' GMM objects, so save_parameter works afterwards.  Returns (mean (D,), var (D,), coeff (M,))."""
        engine = engine or default_engine()
        if isinstance(data, tuple) and len(data) == 2 and np.ndim(data[0]) == 1:
            lens, begin = np.asarray(data[0], dtype=np.int32), np.asarray(data[1], dtype=np.int64)
        else:
            lens = np.array([len(d) for d in data], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d).reshape(-1, self.__vector_size) for d in data], axis=0))
        m = self.__mix_level
        diff = np.zeros((m, 1))
        if differentiation:
            assert 0 <= coefficient <= 1, 'coefficient must lie in [0, 1]'
            rs = np.random if seed is None else np.random.RandomState(seed)
            diff = (rs.random_sample((m, 1)) - rs.random_sample((m, 1))) * coefficient
        units = sorted(unit_hmms)
        e = self.__state_num - 2
        mean, var, _ = engine.flat_start(lens, begin, len(units) * e, m, n_utts=int(len(lens) * proportion), step=step,
                                         coeff=diff[:, 0] if differentiation else None)
        g_mean = mean[None, :].repeat(m, axis=0) + diff * var          # :514, the arithmetic the device repeats per state
        g_var = var[None, :].repeat(m, axis=0)
        for unit in units:
            for k in range(e):
                unit_hmms[unit].profunction[1 + k].set_model(g_mean, g_var, np.ones(m) / m)
        return mean, var, diff[:, 0].copy()

    def mixup_batch(self, unit_hmms, mix_level, perturb=0.2, engine=None):
        """Grow every GMM state of every unit in `unit_hmms` to `mix_level` mixtures by splitting its heaviest mixtures on the device
        (Engine.mixup; the rule: include/poccala_hip.h, pcl_model_mixup) -- what HTK's MU and Kaldi's mix-up do between rounds of EM; the
        reference has no such step (it clusters again when mix_level changes).  The model grown is the engine's when it holds one of the
        units' shape (states unit-major over sorted(unit_hmms), as every batch helper lays them out and flat_start_batch /
        train_segments_batch leave it); otherwise the units' GMM objects are uploaded first.  The grown parameters are written into the
        GMM objects, whose mixture count follows, and this object's mix_level with it, so save_parameter works afterwards and
        train_segments_batch(..., mix_level=None) / estep_batch continue from the grown model without clustering again:
        flat_start_batch at mix_level 1 -> EM -> mixup_batch(2) -> EM -> mixup_batch(4) -> ...  Returns origin (J, mix_level) int32: the
        old mixture every new one descends from."""
        engine = engine or default_engine()
        units = sorted(unit_hmms)
        e = self.__state_num - 2
        gmms = [unit_hmms[u].profunction[1 + k] for u in units for k in range(e)]
        have = (len(gmms), gmms[0].mixture, gmms[0].dimension)
        if any((len(gmms), g.mixture, g.dimension) != have for g in gmms):
            raise ValueError('mixup_batch: the units\' GMM states differ in mixture count or dimension')
        if (engine.J, engine.M, engine.D) != have:
            engine.load_model(*self._model_arrays(unit_hmms)[2])
        origin = engine.mixup(mix_level, perturb=perturb, want_origin=True)
        self._adopt_model(engine.model_download(), units, unit_hmms)
        return origin

    def adapt_batch(self, labels, data_list, unit_hmms, method='mllr', unit_class=None, iterations=1, min_occ=1000.0, tau=10.0,
                    precision=PCL_F32, engine=None):
        """Adapt the units' means to the labelled utterances on the device: per iteration an E-step with the accumulate pass (as
        estep_batch runs it), then method='mllr': Engine.mllr_estimate + transform_means -- unit_class {unit: class} gives every unit a
        regression class (its emitting states inherit it; -1 or a unit left out = not transformed; None = one class of everything) --
        or method='map': Engine.mstep_map(tau).  Variances, weights and transitions stay.  data_list: (T_u, D) arrays, or the
        (lens, begin) of resident frames.  The GMM objects' means follow the device, as in mixup_batch.  Returns a dict:
        logp = per iteration the total ln P(O) of the model the iteration STARTED from, and for MLLR W / occ / status per iteration.
        Transforms of successive iterations are not composed: each is estimated for, and applied to, the current means."""
        if method not in ('mllr', 'map'):
            raise ValueError("adapt_batch: method must be 'mllr' or 'map', got %r" % (method,))
        engine = engine or default_engine()
        keep = self._nonempty(data_list)
        if len(keep) < self._utt_count(data_list):          # empty utterances add nothing to the statistics
            labels, data_list = [labels[u] for u in keep], self._utt_subset(data_list, keep)
        units = sorted(unit_hmms)
        e = self.__state_num - 2
        state_class, n_classes = None, 1
        if method == 'mllr' and unit_class is not None:
            per_unit = np.array([int(unit_class.get(u, -1)) for u in units], dtype=np.int32)
            state_class = np.repeat(per_unit, e)
            n_classes = max(int(per_unit.max()) + 1, 1)
        out = dict(logp=[], W=[], occ=[], status=[])
        for _ in range(int(iterations)):
            b, n, units, idx = self._sentence_batch(labels, data_list, unit_hmms, engine)
            b.score(precision)
            b.forward_backward()
            engine.stats_zero()
            b.accumulate(precision)
            out['logp'].append(float(np.sum(b.get('logp'))))
            b.close()
            if method == 'mllr':
                W, occ, status = engine.mllr_estimate(state_class, n_classes, min_occ)
                engine.transform_means(None, state_class, n_classes)
                out['W'].append(W), out['occ'].append(occ), out['status'].append(status)
            else:
                engine.mstep_map(tau)
            self._adopt_model(engine.model_download(), units, unit_hmms)
        if method == 'map':
            del out['W'], out['occ'], out['status']
        return out

    @staticmethod
    def compose_fmllr(W_run, logdet_run, W_new, logdet_new):
        """The transform that applies W_run and then W_new, per speaker: A <- A_new A, b <- A_new b + b_new, ln|det A| added."""
        A, b = W_run[:, :, 1:], W_run[:, :, 0]
        An, bn = W_new[:, :, 1:], W_new[:, :, 0]
        out = np.concatenate([(np.einsum('sij,sj->si', An, b) + bn)[:, :, None], np.einsum('sij,sjk->sik', An, A)], axis=2)
        return out, np.asarray(logdet_run, dtype=np.float64) + np.asarray(logdet_new, dtype=np.float64)

    def fmllr_batch(self, labels, data_list, unit_hmms, utt_speaker, iterations=1, n_iter=20, min_occ=1000.0, precision=PCL_F64, engine=None,
                    n_speakers=None):
        """fMLLR on the device: one affine transform of the FEATURES per speaker, y = b + A x (Engine.fmllr_estimate; the rule:
        include/poccala_hip.h).  The model stays as it is; the engine's resident frames are transformed in place.  utt_speaker: one
        speaker index >= 0 per utterance, -1 = leave the utterance alone.  Per iteration: an E-step on the current frames (score +
        forward-backward), Batch.accumulate_fmllr, the estimate, Engine.transform_frames; the new transform is composed onto the running
        one on the host (compose_fmllr).  data_list: (T_u, D) arrays (uploaded once, as float64), or the (lens, begin) of resident frames.
        Returns a dict: logp = iterations + 1 totals of ln P(O) + sum_u T_u ln|det A_speaker(u)| -- of the frames as given, then after
        every iteration, so that the entries are comparable --, W (S, D, D+1) / logdet (S,) = the composed transforms, status = per
        iteration the (S,) statuses, q_trace = per iteration (S, n_iter), W_iter = per iteration (W, logdet) as estimated."""
        engine = engine or default_engine()
        spk = np.asarray(utt_speaker, dtype=np.int32).reshape(-1)
        if len(spk) != self._utt_count(data_list) or len(labels) != len(spk):
            raise ValueError('fmllr_batch: one label sequence and one speaker per utterance')
        keep = self._nonempty(data_list)
        if len(keep) < self._utt_count(data_list):          # empty utterances add nothing to the statistics
            labels, data_list, spk = [labels[u] for u in keep], self._utt_subset(data_list, keep), spk[keep]
        S = int(n_speakers) if n_speakers is not None else max(int(spk.max()) + 1, 1)
        res = self._resident(data_list)
        if res is None:                                      # uploaded ONCE: every later pass reads what the last one left resident
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d, dtype=np.float64) for d in data_list], axis=0))
        else:
            lens, begin = res
        D = int(engine.FD)
        W_run = np.stack([np.concatenate([np.zeros((D, 1)), np.eye(D)], axis=1)] * S)
        logdet_run = np.zeros(S)
        out = dict(logp=[], status=[], q_trace=[], W_iter=[])

        def estep():
            b = self._sentence_batch(labels, (lens, begin), unit_hmms, engine)[0]
            b.score(precision)
            b.forward_backward()
            total = float(np.sum(b.get('logp')))
            out['logp'].append(total + float(np.sum(lens * np.where(spk >= 0, logdet_run[np.maximum(spk, 0)], 0.0))))
            return b

        for _ in range(int(iterations)):
            b = estep()
            engine.fmllr_zero(S)
            b.accumulate_fmllr(spk)
            b.close()
            W, logdet, q, status = engine.fmllr_estimate(n_iter, min_occ)
            engine.transform_frames(lens, begin, spk, None, S)
            W_run, logdet_run = self.compose_fmllr(W_run, logdet_run, W, logdet)
            out['status'].append(status), out['q_trace'].append(q), out['W_iter'].append((W, logdet))
        estep().close()
        out['W'], out['logdet'] = W_run, logdet_run
        return out

    def mllt_batch(self, labels, data_list, unit_hmms, iterations=1, n_iter=20, min_occ=1000.0, state_keep=None, precision=PCL_F64, engine=None,
                   c_covariance=1e-3):
        """MLLT on the device: ONE square transform A of the features for all utterances (Engine.mllt_estimate; the rule:
        include/poccala_hip.h), applied to the engine's resident frames AND to the model's means.  The step between lda_batch and
        fmllr_batch.

        Per iteration:
          1. an E-step on the current frames (score + forward-backward) with Batch.accumulate and Batch.accumulate_mllt on the same batch;
          2. the estimate (n_iter row sweeps, refused below min_occ);
          3. Engine.transform_frames and Engine.transform_means with [0 | A] -- the variances are left alone;
          4. a second E-step on the new frames and Engine.mstep(c_covariance), which re-estimates the variances there (c_covariance is
             the M-step's variance floor, as everywhere else).
        The transforms are composed on the host.  The units' GMM objects follow the device after every change.

        state_keep (J,): 0 = the state is left out of the statistics; it is transformed like the others.
        data_list: (T_u, D) arrays (uploaded once, as float64), or the (lens, begin) of resident frames, so that lda_batch -> flat start /
        EM -> mllt_batch uploads no frame.
        Raises ValueError when the two occupancies of an estimate differ by more than 1e-3 relative: the frame side and the statistics
        block did not see the same posteriors.

        Returns a dict:
          logp              iterations + 1 totals of ln P(O) + F ln|det A_composed|: of the model and frames as given, then after every
                            iteration's M-step.  F = the frames the sentence HMMs emit (the E-step's total occupancy), so the entries
                            are comparable.
          logp_transformed  per iteration the same total right after step 3, before the M-step.  It is never below the iteration's logp
                            entry: that is what EM promises of the transform.
          A, logdet         the composed transform (D, D) and its ln|det|.
          A_iter            per iteration the A the estimate gave (A = A_iter[-1] .. A_iter[0]).
          status, q_trace, occ   per iteration what Engine.mllt_estimate returned under these names.
        logp may FALL from the second iteration on.  The M-step sets the variances to second moments, and the reference's log density
        (util.py:29) carries -1/2 sum(var), not -1/2 sum(ln var), in its constant, so those variances do not maximise it.  With a proper
        Gaussian constant both steps would raise it (DESIGN.md section 7 (f13) has the figures)."""
        engine = engine or default_engine()
        if len(labels) != self._utt_count(data_list):
            raise ValueError('mllt_batch: one label sequence per utterance')
        keep = self._nonempty(data_list)
        if len(keep) < self._utt_count(data_list):          # empty utterances add nothing to the statistics
            labels, data_list = [labels[u] for u in keep], self._utt_subset(data_list, keep)
        res = self._resident(data_list)
        if res is None:                                      # uploaded ONCE: every later pass reads what the last one left resident
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d, dtype=np.float64) for d in data_list], axis=0))
        else:
            lens, begin = np.asarray(res[0], dtype=np.int32), np.asarray(res[1], dtype=np.int64)
        D = int(engine.FD)
        A_run, logdet_run = np.eye(D), 0.0
        one = np.zeros(len(lens), dtype=np.int32)
        out = dict(logp=[], logp_transformed=[], status=[], q_trace=[], occ=[], A_iter=[])

        def estep(key):
            b, _, units, _ = self._sentence_batch(labels, (lens, begin), unit_hmms, engine)
            b.score(precision)
            b.forward_backward()
            engine.stats_zero()
            b.accumulate(precision)
            emitted = float(engine.stats_download(moments=False)['acc'].sum())   # every emitted frame carries one ln|det A|
            out[key].append(float(np.sum(b.get('logp'))) + emitted * logdet_run)
            return b, units

        for _ in range(int(iterations)):
            b, units = estep('logp')
            engine.mllt_zero(state_keep)
            b.accumulate_mllt()
            b.close()
            est = engine.mllt_estimate(n_iter, min_occ)
            beta, occ = float(est['occ'][0]), float(est['occ'][1])
            if abs(beta - occ) > 1e-3 * max(abs(beta), abs(occ)):
                raise ValueError('mllt_batch: the frames\' occupancy %.9g and the statistics block\'s %.9g differ by more than 1e-3: the two '
                                 'sides of G did not see the same posteriors' % (beta, occ))
            W = np.concatenate([np.zeros((D, 1)), est['A']], axis=1)[None]
            engine.transform_frames(lens, begin, one, W)
            engine.transform_means(W)
            self._adopt_model(engine.model_download(), units, unit_hmms)
            A_run, logdet_run = est['A'].dot(A_run), logdet_run + est['logdet']
            out['status'].append(est['status']), out['q_trace'].append(est['q_trace']), out['occ'].append(est['occ']), out['A_iter'].append(est['A'])
            b, units = estep('logp_transformed')                       # the statistics of the transformed frames: the variances of the new space
            b.close()
            engine.mstep(c_covariance)
            self._adopt_model(engine.model_download(), units, unit_hmms)
        b, units = estep('logp')
        b.close()
        out['A'], out['logdet'] = A_run, logdet_run
        return out

    def lda_batch(self, labels, data_list, unit_hmms, D_out, left=4, right=4, state_class=None, eps=1e-10, precision=PCL_F64, engine=None):
        """LDA on the device, beside flat_start_batch: forced alignment of the labelled utterances with the units' current model, the class
        statistics of the spliced frames from the Viterbi owner map (Batch.accumulate_lda: every GMM state its own class, or state_class
        (J,) folding tied states), the estimate (Engine.lda_estimate) and the projection (Engine.splice_project) in one call.  Afterwards
        the engine's resident frames are (F, D_out) -- the rows of empty utterances zero -- and the model is of the OLD dimension: start
        again with flat_start_batch at D_out.  data_list: (T_u, D) arrays (uploaded here as float64), or the (lens, begin) of resident
        frames.  Utterances the alignment drops add nothing to the statistics but are projected like the others.  Returns a dict: A
        (D_out, Ds), b (D_out,), eigenvalues (D_out,), n (classes,) rows per class, dropped = the utterances left out of the statistics,
        lens / begin of the projected utterances."""
        engine = engine or default_engine()
        res = self._resident(data_list)
        if res is None:
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d, dtype=np.float64).reshape(len(d), -1) for d in data_list], axis=0))
        else:
            lens, begin = np.asarray(res[0], dtype=np.int32), np.asarray(res[1], dtype=np.int64)
        keep = [u for u in range(len(lens)) if lens[u] > 0]
        b = self._sentence_batch([labels[u] for u in keep], (lens[keep], begin[keep]), unit_hmms, engine)[0]
        try:
            b.score(precision)
            b.viterbi()
            R = int(engine.J) if state_class is None else int(np.max(state_class)) + 1
            engine.lda_zero(max(R, 1), left, right)
            b.accumulate_lda(state_class)
            seg, dropped = b.align_segments()                 # (only for the list of utterances its drop rule leaves out)
            seg.close()
        finally:
            b.close()
        A, bias, lam = engine.lda_estimate(D_out, eps)
        n = engine.lda_stats()[0]
        engine.splice_project(lens, begin, left, right, A, bias)
        gone = sorted(set(range(len(lens))) - set(keep)) + [keep[u] for u in dropped]
        return dict(A=A, b=bias, eigenvalues=lam, n=n, dropped=sorted(gone), lens=lens, begin=begin)

    def cmvn_batch(self, lens, begin=None, utt_speaker=None, norm_vars=True, var_floor=1e-20, min_count=1, engine=None):
        """CMVN on the device, in front of lda_batch / mllt_batch / fmllr_batch: Engine.cmvn_zero + cmvn_accumulate + cmvn_apply in one call on
        the engine's resident frames, which are normalised in place (the rule: include/poccala_hip.h).  (lens, begin): the utterances of
        resident frames (Engine.frontend / load_audio_batch(fetch=False)), also as one tuple in `lens`; or `lens` a list of (T_u, D)
        arrays, uploaded here as float64 and laid back to back.  utt_speaker: one speaker index >= 0 per utterance, -1 = leave the
        utterance alone, None = every utterance by its own statistics.  Returns a dict: status (S,) int32 (0, or why the speaker was
        left alone: 1 fewer than min_count frames, 2 a sum that is not finite), n (S,) frames per speaker, lens / begin of the utterances."""
        engine = engine or default_engine()
        res = self._resident(lens) if begin is None else (np.asarray(lens, dtype=np.int32).reshape(-1), np.asarray(begin, dtype=np.int64).reshape(-1))
        if res is None:
            data_list = lens
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d, dtype=np.float64).reshape(len(d), -1) for d in data_list], axis=0))
        else:
            lens, begin = res
        spk = np.arange(len(lens), dtype=np.int32) if utt_speaker is None else np.asarray(utt_speaker, dtype=np.int32).reshape(-1)
        if len(spk) != len(lens):
            raise ValueError('cmvn_batch: one speaker per utterance')
        S = max(int(spk.max()) + 1, 1)
        engine.cmvn_zero(S)
        engine.cmvn_accumulate(lens, begin, spk)
        n = engine.cmvn_stats()[0]
        status = engine.cmvn_apply(lens, begin, spk, norm_vars, var_floor, min_count, S)
        return dict(status=status, n=n, lens=lens, begin=begin)

    def _adopt_model(self, model, units, unit_hmms):
        """(mean, var, weight) of a model laid out unit-major over `units` into the units' GMM objects; this object's mix_level follows."""
        mean, var, w = model
        e = self.__state_num - 2
        for ui, unit in enumerate(units):
            for k in range(e):
                unit_hmms[unit].profunction[1 + k].set_model(mean[ui * e + k], var[ui * e + k], w[ui * e + k])
        self.__mix_level = int(mean.shape[1])

    def init_segments_batch(self, labels, data_list, unit_hmms, mix_level=None, c_covariance=1e-3, seed=0, precision=PCL_F64, engine=None):
        """The first round of training scheme 1, which needs no model: uniform segmentation (multi_process_data(init=True),
        AcousticModel.py:734-735: every utterance cut into equal chunks, one per label unit; __get_gmmdata :629-644: every chunk into
        S-2 slices) on the device, then clustering + stand-alone EM of every GMM state as train_segments_batch(init=True) runs them
        -- but WITHOUT its forced alignment, which would need a model.  mix_level defaults to this object's.  Returns what
        train_segments_batch returns, {unit: (iters (S-2,), q (S-2,), skipped (S-2,) bool)}; the units' GMM objects receive the new
        parameters and the engine holds the model.  `data_list` as for train_segments_batch: host arrays, or (lens, begin) of resident
        frames.  An utterance without frames adds nothing.  The reference also runs the SMEM split /
        merge on this round (smem=init, :835): outside the hot path here, as for train_segments_batch."""
        engine = engine or default_engine()
        keep = self._nonempty(data_list)
        labels, data_list = [labels[u] for u in keep], self._utt_subset(data_list, keep)
        units = sorted(unit_hmms)
        idx = {u: i for i, u in enumerate(units)}
        e = self.__state_num - 2
        res = self._resident(data_list)
        if res is not None:                                  # frames already resident: nothing is uploaded
            lens, begin = res
        else:
            lens = np.array([len(d) for d in data_list], dtype=np.int32)
            begin = np.concatenate([[0], np.cumsum(lens[:-1].astype(np.int64))]).astype(np.int64)
            engine.load_frames(np.concatenate([np.asarray(d) for d in data_list], axis=0))
        unit_ids = [np.array([idx[u] for u in lab], dtype=np.int32) for lab in labels]
        seg = engine.uniform_segments(unit_ids, lens, begin, e, len(units) * e)
        k = int(mix_level) if mix_level is not None else self.__mix_level
        return self._train_segments(engine, seg, units, unit_hmms, True, k, False, c_covariance, seed, precision)

    def train_segments_data(self, unit_data, unit_hmms, init=False, mix_level=None, smem=False, c_covariance=1e-3, seed=0,
                            precision=PCL_F64, engine=None):
        """The same from already regrouped data, {unit: [S-2 arrays (n_k, D)]} (what `regroup_batch` returns and what
        multi_training reads back from <unit>/data, AcousticModel.py:790-797); a unit without data is skipped."""
        self._no_smem(smem)
        engine = engine or default_engine()
        units, idx, (mean, var, w), trans = self._model_arrays(unit_hmms)
        e = self.__state_num - 2
        blocks, state = [], []
        for ui, unit in enumerate(units):
            for kk, block in enumerate(unit_data.get(unit, [])):
                block = np.asarray(block, dtype=np.float64)
                if len(block):
                    blocks.append(block)
                    state.append(np.full(len(block), ui * e + kk, dtype=np.int32))
        if not blocks:                                                # no unit has data: every state is skipped, nothing touches the GPU
            self.last_segment_counts = {unit: np.zeros(e, dtype=np.int32) for unit in units}
            return {unit: (np.full(e, -1, dtype=np.int32), np.full(e, np.nan), np.ones(e, dtype=bool)) for unit in units}
        engine.load_model(mean, var, w)
        engine.load_frames(np.concatenate(blocks, axis=0))
        seg = engine.segments(np.concatenate(state))
        return self._train_segments(engine, seg, units, unit_hmms, init, mix_level, smem, c_covariance, seed, precision)

    # ------------------------------------------------------------------ the reference's two workers, at batched speed
    # The reference fans its corpus out over a Pool, one call per utterance (AcousticModel.py:861-870, :709-712): every call
    # builds one LHMM per label position, scores, embeds, runs Baum-Welch / Viterbi and writes files.  Called like that, one
    # utterance at a time, a GPU sees 300 frames per launch (extra.zero_change_route: ~5 k frames/s).  The two methods below keep
    # the reference's signatures and file outputs but DEFER the work: a call queues (label, data); flush_workers() -- called by
    # the caller after its loop, and by itself every `flush_frames` frames -- runs everything queued as one batch through
    # estep_batch / segment_batch and writes what the per-utterance workers would have written, merged per unit:
    #   multi_embedded_training_1 -> <unit>/HMM/{ksai-acc,gamma-acc}/*.npy, <unit>/GMM_k/{acc,alpha-acc,mean-acc,covariance-acc}/*.npy
    #                                (one file set per unit and flush instead of one per utterance x label position; the merge of
    #                                 multi_embedded_training_2 -- LHMM.init_acc / GMM.init_acc, a log-sum-exp over the files --
    #                                 gives the same sums)
    #   multi_process_data        -> <unit>/data/*.pkl, one pickle per contiguous run of the unit (AcousticModel.__save_data)
    # No Pool, no Controller: only these two entry points.
    def _worker_units(self, units, init):
        if self.worker_units is not None:
            return {u: self.worker_units[u] for u in units}
        out = {}
        for u in units:                          # init_unit + init_parameter ONCE per unit and flush (the reference: per label position)
            hmm = self.init_unit(unit=u, new_log=init)
            self.init_parameter(unit=u, hmm=hmm)
            out[u] = hmm
        return out

    def _enqueue(self, kind, item):
        """Queue one worker call.  The data are COPIED (the reference's Pool pickles them at call time, AcousticModel.py:865-870: a caller
        may refill its feature buffer right after the call).  Inside a multiprocessing worker (the reference's own pattern:
        pool.apply_async(self.multi_embedded_training_1, ...)) the process may end with the task, and multiprocessing children leave
        through os._exit without running atexit handlers, so nothing is deferred there: the call is flushed at once (the
        per-utterance rate; the batched rate needs the calls made from one process), with one warning."""
        import multiprocessing as mp
        self.__queued[kind].append(item)
        self.__queued_frames += len(item[1])
        if not self.__flush_registered:
            import atexit
            import weakref
            ref = weakref.ref(self)
            atexit.register(lambda: ref() is not None and ref()._flush_at_exit())
            self.__flush_registered = True
        if mp.parent_process() is not None:
            if not self.__warned_worker:
                import warnings
                warnings.warn('poccala_amd.AcousticModel: multi_embedded_training_1 / multi_process_data called inside a multiprocessing worker; '
                              'the deferred batch cannot outlive the task, so every call is flushed at once (one utterance per launch chain). '
                              'Call the workers from one process and flush_workers() after the loop for the batched rate.', RuntimeWarning)
                self.__warned_worker = True
            self.flush_workers()
        elif self.__queued_frames >= self.flush_frames:
            self.flush_workers()

    def _flush_at_exit(self):
        """atexit: whatever is still queued is run and written (with a warning: the caller forgot flush_workers())."""
        if self.__queued['train'] or self.__queued['align']:
            import warnings
            warnings.warn('poccala_amd.AcousticModel: %d queued worker calls were still waiting at interpreter exit; flushing them now '
                          '(call flush_workers() after the loop)' % (len(self.__queued['train']) + len(self.__queued['align'])), RuntimeWarning)
            try:
                self.flush_workers()
            except Exception as e:             # noqa: the interpreter is going down; say what is lost
                warnings.warn('poccala_amd.AcousticModel: the exit flush failed, the queued accumulators are LOST: %r' % (e,), RuntimeWarning)

    def __del__(self):
        try:
            q = self.__queued
        except AttributeError:
            return
        if q['train'] or q['align']:
            import warnings
            warnings.warn('poccala_amd.AcousticModel: dropped with %d queued worker calls that were never flushed (flush_workers()): their '
                          'accumulator / data files were NOT written' % (len(q['train']) + len(q['align'])), RuntimeWarning)

    def multi_embedded_training_1(self, label, data, init, *args):
        """AcousticModel.multi_embedded_training_1(label, data, init, show_q, load_num, file_count, fix_code)
        (AcousticModel.py:884-916), deferred: see flush_workers."""
        fix_code = int(args[3]) if len(args) > 3 else 0
        self._enqueue('train', (list(label), np.array(data, copy=True), bool(init), fix_code))

    def multi_process_data(self, label, data, init, *args):
        """AcousticModel.multi_process_data(label, data, init, load_num, file_count, fix_code) (AcousticModel.py:723-768):
        init -> the utterance is cut into equal chunks per label unit at once (__eq_segment mode 'e', host work); otherwise the
        forced alignment is deferred: see flush_workers."""
        if init:
            self.eq_segment(np.asarray(data), list(label), mode='e', save=self.save_data)
            return
        self._enqueue('align', (list(label), np.array(data, copy=True), False, 0))

    def save_data(self, unit, unit_data):
        """AcousticModel.__save_data (AcousticModel.py:331-351): one pickle per block under <unit>/data/ (the reference names the
        file by pid and second, so two blocks of one second overwrite each other; a running number is appended here)."""
        import pickle
        import time
        path = self.unit_path(unit) + '/data'
        os.makedirs(path, exist_ok=True)
        self.__data_files += 1
        with open('%s/%s_data_%s_%s_%06d.pkl' % (path, unit, os.getpid(), int(time.time()), self.__data_files), 'wb') as f:
            pickle.dump(unit_data, f, protocol=pickle.HIGHEST_PROTOCOL)

    def flush_workers(self):
        """Run everything multi_embedded_training_1 / multi_process_data queued, as batches.  Returns
        {'train': (utterances, frames, logp array), 'align': (utterances, frames, dropped utterance indices)}."""
        out = {}
        queued, self.__queued = self.__queued, {'train': [], 'align': []}
        self.__queued_frames = 0
        eng = self.worker_engine
        if queued['train']:
            lp_all, n_utt, n_fr = [], 0, 0
            # one E-step per (fix_code, init): fix_code decides what is accumulated, init whether the unit logs start afresh
            # (init_unit(new_log=init), AcousticModel.py:897) -- every queued call keeps its own flag
            # groups in the order their first call was queued (the reference applies `init` per call, in call order: a first call with
            # init=True must restart the unit logs BEFORE the later init=False calls write to them -- ADVICE r5: sorted() ran False first)
            for fix_code, init in dict.fromkeys((q[3], q[2]) for q in queued['train']):
                part = [q for q in queued['train'] if q[3] == fix_code and q[2] == init]
                labels, datas = [q[0] for q in part], [q[1] for q in part]
                units = self._worker_units(sorted({u for lab in labels for u in lab}), init)
                stats, hmm_acc, logp = self.estep_batch(labels, datas, units, fix_code=fix_code,
                                                        precision=PCL_F32 if self.worker_precision is None else self.worker_precision, engine=eng)
                self.save_batch_acc(stats, hmm_acc, units)
                lp_all.append(logp)
                n_utt += len(part)
                n_fr += int(sum(len(d) for d in datas))
            out['train'] = (n_utt, n_fr, np.concatenate(lp_all))
        if queued['align']:
            labels, datas = [q[0] for q in queued['align']], [q[1] for q in queued['align']]
            units = self._worker_units(sorted({u for lab in labels for u in lab}), False)
            blocks, dropped = self.segment_batch(labels, datas, units, precision=PCL_F64 if self.worker_precision is None else self.worker_precision,
                                                 engine=eng)
            for unit, runs in blocks.items():                                   # AcousticModel.py:758-764
                for run in runs:
                    self.save_data(unit, run)
            for u in dropped:
                self.log.note('viterbi切分失败', cls='w')                         # AcousticModel.py:755 (the utterance is discarded)
            out['align'] = (len(labels), int(sum(len(d) for d in datas)), dropped)
        return out

    def save_batch_acc(self, stats, hmm_acc, unit_hmms):
        """Write the result of `estep_batch` as reference-format accumulator files (log domain, float64,
        SURVEY T3): <unit>/HMM/{ksai-acc,gamma-acc}/..., <unit>/GMM_k/{acc,alpha-acc,mean-acc,covariance-acc}/...
        so that the reference's multi_embedded_training_2 (AcousticModel.py:918-935) can merge them."""
        units = sorted(unit_hmms)
        e = self.__state_num - 2
        if stats is not None:
            with np.errstate(divide='ignore'):                          # ln 0 = -inf for a state no frame reached
                ln = {k: np.log(stats[k]) for k in ('acc', 'alpha_acc', 'mean_acc', 'cov_acc')}
        for ui, unit in enumerate(units):
            hmm = unit_hmms[unit]
            touched = False
            # the files hold THIS batch's accumulators only (the reference writes one set per utterance from fresh unit
            # objects, AcousticModel.py:897-913): start from ln 0, or a second call would save batch 1 + batch 2 and the
            # merge (init_acc) would count batch 1 twice
            hmm.reset_acc()
            if unit in hmm_acc:
                hmm.add_acc(hmm_acc[unit][0], hmm_acc[unit][1])
                touched = True
            if stats is not None:
                for k in range(e):
                    j = ui * e + k
                    g = hmm.profunction[1 + k]
                    g.acc = ln['acc'][j]
                    g.alpha_acc = float(ln['alpha_acc'][j])
                    g.mean_acc = ln['mean_acc'][j]
                    g.covariance_acc = ln['cov_acc'][j]
                    touched = touched or stats['alpha_acc'][j] > 0
            if touched:
                self.save_acc(unit, hmm)
                hmm.reset_acc()
