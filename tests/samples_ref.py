"""NumPy restatement of cdc_sample_moments (include/cdc_hip.h: THE WELFORD ORDER): the sequential update in float32, every operation
rounded on its own, and the float64 mean / unbiased variance it is measured against."""
import numpy as np

F = np.float32


def welford32(samples, count_before=0, mean=None, m2=None):
    """samples [K, ...] float32, folded in the order k = 0 .. K-1 onto (mean, m2) at count_before -> (mean, m2) float32.
    NumPy's float32 arithmetic rounds every operation to float32 (IEEE, division included), which is the kernel's contract."""
    x = np.asarray(samples, F)
    mean = np.zeros(x.shape[1:], F) if count_before == 0 else np.array(mean, F)
    m2 = np.zeros(x.shape[1:], F) if count_before == 0 else np.array(m2, F)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            cnt = F(count_before + k + 1)
            d = x[k] - mean
            mean = mean + d / cnt
            m2 = m2 + d * (x[k] - mean)
    assert mean.dtype == F and m2.dtype == F
    return mean, m2


def mean_var32(samples):
    """(mean, unbiased variance) of samples [K, ...] as the library returns them: welford32, then m2 / float32(K - 1)."""
    mean, m2 = welford32(samples)
    K = np.asarray(samples).shape[0]
    with np.errstate(all="ignore"):
        return mean, (m2 / F(K - 1)).astype(F) if K >= 2 else m2


def mean_var64(samples):
    """The float64 mean and unbiased variance (two-pass) of samples [K, ...]."""
    x = np.asarray(samples, np.float64)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).sum(axis=0) / (x.shape[0] - 1) if x.shape[0] >= 2 else np.zeros_like(mean)
    return mean, var
