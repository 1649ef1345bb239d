"""The reference box filter of include/rt_capi_ssaa.h, in numpy: what k x k supersampling must compute from a virtual
kW x kH frame (the oracle's, or the GPU's own rt_render)."""
import numpy as np


def box_filter(virtual, k):
    """virtual: float32 (k*X, k*H, 3), pixels[x][z] order -> float32 (X, H, 3).  Output pixel (x, z) is the fp32 sum of
    virtual pixels (k*x + i, k*z + j) in the order s = i*k + j, strictly sequential, divided by k*k."""
    assert virtual.dtype == np.float32 and virtual.shape[0] % k == 0 and virtual.shape[1] % k == 0
    X, H = virtual.shape[0] // k, virtual.shape[1] // k
    v = virtual.reshape(X, k, H, k, 3)                 # [x, i, z, j, c]
    acc = v[:, 0, :, 0].copy()
    for s in range(1, k * k):
        i, j = divmod(s, k)
        acc = acc + v[:, i, :, j]                      # float32 + float32: one fp32 rounding per add
    return acc / np.float32(k * k)
