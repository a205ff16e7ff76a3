"""NumPy twin of csrc/model_mixup.hip: the mix-up rule of include/poccala_hip.h (pcl_model_mixup), float64, one rounded operation at a
time.  Written from the rule, not from the kernels: it walks the rounds on the whole model, the device plans on the weights and replays
the rounds per element.  The GPU tests compare the device with `mixup` on random models."""
import numpy as np

M_MAX = 8192


def mixup(mean, var, weight, M_new, perturb=0.2):
    """(mean (J,M_new,D), var (J,M_new,D), weight (J,M_new), origin (J,M_new) int32) of the grown model.  Raises ValueError for what the
    library refuses: M_new <= M, M_new > 8192, a negative or non-finite perturb, a state without a mixture of weight > 0."""
    mean, var, weight = (np.asarray(a, dtype=np.float64) for a in (mean, var, weight))
    J, M, D = mean.shape
    M_new = int(M_new)
    if not M < M_new <= M_MAX:
        raise ValueError('mixup: M_new = %d, need more than %d and at most %d' % (M_new, M, M_MAX))
    if not (np.isfinite(perturb) and perturb >= 0):
        raise ValueError('mixup: perturb = %r' % (perturb,))
    perturb = np.float64(perturb)
    mu, vr = np.zeros((J, M_new, D)), np.ones((J, M_new, D))
    w, origin = np.zeros((J, M_new)), np.zeros((J, M_new), dtype=np.int32)
    mu[:, :M], vr[:, :M], w[:, :M] = mean, var, weight
    origin[:, :M] = np.arange(M)
    for j in range(J):
        if not (weight[j] > 0).any():                                # checked for every state before anything is changed
            raise ValueError('mixup: state %d has no live mixture' % j)
    for j in range(J):
        cur = M
        while cur < M_new:
            live = np.flatnonzero(w[j, :cur] > 0)                    # (NaN > 0 is False)
            if len(live) == 0:                                       # every weight has been halved to zero: the rule could not end
                raise ValueError('mixup: state %d has no live mixture' % j)
            n = min(M_new - cur, len(live))
            order = live[np.argsort(-w[j, live], kind='stable')]     # weight descending, equal weights by ascending index
            parents, kids = order[:n], cur + np.arange(n)            # distinct slots: the round's updates do not meet
            delta = perturb * np.sqrt(vr[j, parents])
            before = mu[j, parents]                                  # (a copy: both updates start from the mean before this round)
            mu[j, kids] = before + delta
            mu[j, parents] = before - delta
            vr[j, kids] = vr[j, parents]
            h = 0.5 * w[j, parents]
            w[j, parents] = h
            w[j, kids] = h
            origin[j, kids] = origin[j, parents]
            cur += n
    return mu, vr, w, origin
