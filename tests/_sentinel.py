"""Helpers of the ragged-size GPU tests: device buffers with 512 elements of excess behind every array (1e30 behind inputs, NaN behind
cotangents, -7.25 behind outputs) and the check that the excess comes back bit-identical; the 4 x float32-deviation gate of
tests/test_gpu_likelihood.py with its `ERR <case> <value> gate <gate>` line."""
import numpy as np

PAD, SENTINEL = 512, -7.25


class Buffers:
    def __init__(self):
        self.kept = []

    def _make(self, a, fill):
        import torch
        a = np.ascontiguousarray(a)
        if np.iscomplexobj(a):      # a half-spectrum travels as float pairs: 512 floats of excess
            flat = a.reshape(-1).view(np.float32 if a.dtype == np.complex64 else np.float64)
            return torch.view_as_complex(self._make(flat, fill).reshape(-1, 2)).reshape(a.shape)
        full = np.full((a.shape[0] + PAD,) + a.shape[1:], fill, dtype=a.dtype)
        full[:a.shape[0]] = a
        base = torch.from_numpy(full).cuda()
        self.kept.append((base, a.shape[0], base[a.shape[0]:].clone()))
        return base[:a.shape[0]]

    def inp(self, a, fill=1e30):      # read-only input; a bool mask's excess is True
        return self._make(a, True if np.asarray(a).dtype == bool else fill)

    def cot(self, a):      # cotangent input: NaN behind the end
        return self._make(a, np.nan)

    def out(self, shape, dtype=np.float32, init=None):      # output, or accumulator holding `init`
        a = np.full(shape, SENTINEL, dtype=dtype) if init is None else np.asarray(init, dtype=dtype).reshape(shape)
        return self._make(a, SENTINEL)

    def check_tails(self):
        import torch
        for base, n, tail in self.kept:
            assert torch.equal(base[n:].contiguous().view(torch.uint8), tail.view(torch.uint8)), "the excess behind an array changed"


def dev_sum(c32, c64):
    """Deviation of a float64 sum of float32 terms, row by row: the sum of the absolute per-term deviations.  Per-term errors of one sign add
    up n times over, not sqrt(n) (a device transcendental against libm's, a rounded constant entering every term alike; csrc/likelihood.hip
    describes the effect on the shash value), and whether they do differs between the device and numpy, so nothing smaller than the sum of
    |d_i| bounds what the same float32 arithmetic in another order may give.  A lost or doubled workgroup partial is hundreds of whole terms,
    each 1e6 .. 1e7 times its own deviation."""
    d = (np.asarray(c32, dtype=np.float64) - c64).reshape(c64.shape[0], -1)
    return np.abs(d).sum(1)


def dev_max(a32, a64):
    return float(np.max(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64))))


def gate(errs, name, got, want, dev, factor=4):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), name
    err = float(np.max(np.abs(got - np.asarray(want, dtype=np.float64))))
    print(f"ERR {name} {err:.3e} gate {factor * float(dev):.3e}")
    if not err <= factor * float(dev):
        errs.append(f"{name}: {err:.3e} > {factor * float(dev):.3e}")


def equal(a, b):
    import torch
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))
