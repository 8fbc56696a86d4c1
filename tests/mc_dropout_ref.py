"""Reference statements for the Monte-Carlo pose heads (csrc/mc_heads.hip, csrc/philox.h), none of which runs project code:
Philox4x32-10 in numpy integers, the mask of (seed, draw, ids, column, sample), and the samples / mean / variance in float64 and
in fp32 torch (the CPU statement whose error the kernel's is compared with)."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
NODE_TAG = 0xFFFFFFFF
_MASK32 = np.uint64(0xFFFFFFFF)
_SH = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (broadcast against each other) of 32-bit values held in uint64: -> uint32 [..., 4]."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & _MASK32 for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> _SH) ^ c1 ^ k0, p1 & _MASK32, (p0 >> _SH) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + np.uint64(W0)) & _MASK32, (k1 + np.uint64(W1)) & _MASK32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def mask_words(seed, draw, a, b, k, s):
    """The four words of column chunk k, sample s of the row with ids (a, b): key = (seed low, seed high), counter = (a, b,
    k | s << 16, draw)."""
    seed = int(seed)
    c2 = np.asarray(k, dtype=np.uint64) | (np.asarray(s, dtype=np.uint64) << np.uint64(16))
    return philox4x32_10(a, b, c2, int(draw) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)


def threshold(p: float) -> int:
    return int(np.floor(np.float64(p) * 4294967296.0))


def mask(seed, draw, a, b, d, S, p):
    """keep [S, R, d] (bool): a, b integer arrays [R] (b = NODE_TAG for a node row); element j of chunk k is kept iff word[j] >= T."""
    a, b = np.asarray(a, dtype=np.uint64).reshape(1, -1, 1), np.asarray(b, dtype=np.uint64).reshape(1, -1, 1)
    k = np.arange(d // 4, dtype=np.uint64).reshape(1, 1, -1)
    s = np.arange(S, dtype=np.uint64).reshape(-1, 1, 1)
    w = mask_words(seed, draw, a, b, k, s)                              # [S, R, d/4, 4]
    return (w >= np.uint32(threshold(p))).reshape(S, w.shape[1], d)


def scale_f32(p: float) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def masked_input64(x: torch.Tensor, keep: np.ndarray, p: float) -> torch.Tensor:
    """float64 [S, R, d]: where(keep, x, 0) times the fp32 scale -- the input on which the heads are a plain Linear."""
    xm = torch.where(torch.from_numpy(keep), x.double().unsqueeze(0), torch.zeros((), dtype=torch.float64))
    return xm * float(scale_f32(p))


def statement64(x, w6, b6, keep, p):
    """(samples [S, R, 6], mean [R, 6], var [R, 6]) in float64; var unbiased, zeros for S = 1."""
    z = masked_input64(x, keep, p) @ w6.double().t() + b6.double()
    S = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).sum(0) / (S - 1) if S > 1 else torch.zeros_like(mean)
    return z, mean, var


def statement32(x, w6, b6, keep, p):
    """The same in fp32 torch, as the header states it: scale applied once to the fp32 sum, the mean from the sequential fp32 sum in
    sample order, the variance in two passes."""
    xm = torch.where(torch.from_numpy(keep), x.unsqueeze(0), torch.zeros((), dtype=torch.float32))
    y = torch.from_numpy(np.asarray(scale_f32(p))) * (xm @ w6.t()) + b6
    S = y.shape[0]
    total = torch.zeros_like(y[0])
    for s in range(S):
        total = total + y[s]
    mean = total / S
    ss = torch.zeros_like(mean)
    for s in range(S):
        ss = ss + (y[s] - mean) ** 2
    var = ss / (S - 1) if S > 1 else torch.zeros_like(mean)
    return y, mean, var
