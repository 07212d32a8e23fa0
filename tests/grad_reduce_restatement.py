"""Numpy restatement of the gradient exchange's two kernels (csrc/grad_reduce.hip), every step named.

    pack:    the tensors' elements one after the other (a concatenation), into the front of a row
    reduce:  s = 0.0 (float64); for r = 0 .. W - 1: s += float64(rows[r]); mean = s / float64(W); out = float32(mean)

Conversions float32 -> float64 are exact; the additions, the one division and the one rounding to float32 are IEEE operations
(round to nearest even), on the host as in the kernels - so the kernels are held to EQUAL BITS, not to a tolerance.  (IEEE 754
leaves the sign and payload of a NaN that an operation generates open; inputs of the GPU tests carry quiet NaNs of numpy's own
pattern, which every operation here passes on, and never +Inf and -Inf in one column.)

`kernels()` hands the two functions out under the operators' names for `parallel.GradientAverager(kernels=...)` on CPU tensors."""
import numpy as np

C = 1024            # elements per workgroup (NWS_ADAM_CHUNK)
TABLE = 64          # tensors per launch (NWS_ADAM_TABLE)
MAX_WORLD = 1024    # NWS_GRAD_MAX_WORLD


def pack(tensors):
    """float32 arrays of any shape -> their elements in order, one float32 vector"""
    return np.concatenate([np.asarray(t, dtype=np.float32).reshape(-1) for t in tensors])


def reduce(rows, n=None):
    """rows (W, stride) float32 -> the mean of the first n columns in rank order (n = None: all of them), float32"""
    rows = np.asarray(rows, dtype=np.float32)
    W, stride = rows.shape
    n = stride if n is None else int(n)
    if W == 1:
        return rows[0, :n].copy()           # the row's own bits
    s = np.zeros(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        for r in range(W):
            s = s + rows[r, :n].astype(np.float64)
        return (s / np.float64(float(W))).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


class _Kernels:
    """grad_pack / grad_reduce of the bindings on CPU torch tensors, through the functions above"""

    @staticmethod
    def grad_pack(tensors, out):
        import torch

        flat = pack([t.detach().numpy() for t in tensors])
        assert out.dim() == 1 and out.numel() >= flat.size
        out[:flat.size] = torch.from_numpy(flat)

    @staticmethod
    def grad_reduce(rows, out):
        import torch

        out.copy_(torch.from_numpy(reduce(rows.numpy(), out.numel())))


def kernels():
    return _Kernels()
