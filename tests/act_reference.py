"""CPU references and test inputs shared by tests/test_act_build.py (exemption budgets) and tests/test_act_gpu.py (the kernel):
fp64 softmax statistics, fp64 inverse-CDF bins and the (row, dimension) pairs a comparison has to leave out because the answer is
decided below fp32 resolution."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("pose0_position", "pose0_rotation", "pose1_position", "pose1_rotation")
KEY_DIMS = (2, 4, 2, 4)
KEY_FIRST = (0, 2, 6, 8)
BINS = (50, 100, 50, 50, 50, 50, 50, 100, 50, 50, 50, 50)
OFFS = tuple(int(x) for x in np.concatenate([[0], np.cumsum(BINS)]))
GOLDENS = ("cfg1_T1", "cfg1_T2", "cfg2_20M", "bench_200M", "baseline_gpt", "baseline_gato", "baseline_flamingo")
MODE_GAP = 1e-6        # two largest logits closer than this: fp32 exp rounds both probabilities alike, argmax(probs) is a tie artefact
CDF_MARGIN = 1e-5      # u closer than this to an fp64 cumulative boundary: the fp32 cumulative sum may fall on either side
SCALES = (0.1, 1.0, 4.0)
SAMPLE_ROWS = 1024


def golden_logits(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    modes = z["modes"].reshape(-1, 12) if "modes" in z.files else None
    return z["raw_logits"].reshape(-1, 700).astype(np.float32), modes


def segments(x):
    """[R,700] -> list of 12 arrays [R, n]"""
    return [x[:, OFFS[d]:OFFS[d + 1]] for d in range(12)]


def random_logits(scale, rows=SAMPLE_ROWS, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + int(scale * 10))
    return (torch.randn(rows, 700, generator=g) * scale).numpy().astype(np.float32)


def random_uniforms(rows=SAMPLE_ROWS, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.rand(rows, 12, generator=g).numpy().astype(np.float32)


def argmax_bins(x):
    return np.stack([s.argmax(axis=1) for s in segments(x)], axis=1)


def mode_exempt(x):
    """[R,12] bool: the two largest logits of the segment differ by at most MODE_GAP"""
    out = []
    for s in segments(x):
        top = np.sort(s.astype(np.float64), axis=1)
        out.append(top[:, -1] - top[:, -2] <= MODE_GAP)
    return np.stack(out, axis=1)


def stats64(x, bins):
    """fp64 per-KEY log-probability of `bins` [R,12] and entropy: two arrays [R,4]"""
    lp, en = np.zeros((x.shape[0], 12)), np.zeros((x.shape[0], 12))
    for d, s in enumerate(segments(x)):
        s = s.astype(np.float64)
        m = s.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(s - m).sum(axis=1, keepdims=True))
        logp = s - lse
        lp[:, d] = np.take_along_axis(logp, bins[:, d:d + 1], axis=1)[:, 0]
        en[:, d] = -(np.exp(logp) * logp).sum(axis=1)
    key = lambda a: np.stack([a[:, f:f + w].sum(axis=1) for f, w in zip(KEY_FIRST, KEY_DIMS)], axis=1)
    return key(lp), key(en)


def cdf64(x):
    out = []
    for s in segments(x):
        s = s.astype(np.float64)
        e = np.exp(s - s.max(axis=1, keepdims=True))
        out.append(np.cumsum(e, axis=1) / e.sum(axis=1, keepdims=True))
    return out


def sample_bins64(x, u):
    """fp64 inverse-CDF bins [R,12] and the exemption mask [R,12] (u within CDF_MARGIN of some cumulative boundary)"""
    bins, exempt = [], []
    for d, c in enumerate(cdf64(x)):
        ud = u[:, d:d + 1].astype(np.float64)
        bins.append(np.minimum((c <= ud).sum(axis=1), BINS[d] - 1))
        exempt.append((np.abs(c - ud) <= CDF_MARGIN).any(axis=1))
    return np.stack(bins, axis=1), np.stack(exempt, axis=1)


def sample_bins32_sequential(x, u):
    """the same in fp32 with a sequential cumulative sum (np.cumsum accumulates in the array's type, left to right)"""
    bins = []
    for d, s in enumerate(segments(x)):
        e = np.exp(s - s.max(axis=1, keepdims=True)).astype(np.float32)
        c = np.cumsum(e, axis=1, dtype=np.float32) / e.sum(axis=1, keepdims=True, dtype=np.float32)
        bins.append(np.minimum((c <= u[:, d:d + 1]).sum(axis=1), BINS[d] - 1))
    return np.stack(bins, axis=1)


def de_discretize_cpu(bins):
    """VIMAPolicy._de_discretize_actions on CPU tensors (true fp32 division by 50 / 100) -> [R,12] float32"""
    b = torch.from_numpy(bins.astype(np.int64)).float()
    return (b / torch.tensor(BINS, dtype=torch.float32)).numpy()


def rescale_cpu(bins, low, high):
    """the torch expressions of examples/reference_loop.py (cont * (high - low) + low, clamp; cont * 2 - 1, clamp) on CPU tensors"""
    b = torch.from_numpy(bins.astype(np.int64)).float()
    low, high = torch.tensor([low], dtype=torch.float32), torch.tensor([high], dtype=torch.float32)
    out = torch.empty(b.shape[0], 12)
    for f, w in zip(KEY_FIRST, KEY_DIMS):
        c = b[:, f:f + w].clone()
        if w == 2:
            c[..., 0] = c[..., 0] / 50
            c[..., 1] = c[..., 1] / 100
            c = torch.clamp(c * (high - low) + low, min=low, max=high)
        else:
            c = c / 50
            c = torch.clamp(c * 2 - 1, min=-1, max=1)
        out[:, f:f + w] = c
    return out.numpy()
