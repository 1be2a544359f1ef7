"""Long-form policy (BASELINE config 5; not in the reference, which samples one ``(1, L)`` clip per call, testing/tester.py:153).

Default = UN-CHUNKED: the whole utterance goes through the sampler in one piece -- with the flash attention kernel the 30 s case needs
no 905 MB attention matrix and fits the 288 GB of one MI355X many times over (profiles/DESIGN_history_r01-r04.md section 5, "Long form").  For inputs beyond what one GPU
should hold, or to turn one very long recording into a batch (utterance-parallel over chunks, also across ranks), the clip is cut into
equal-length, overlapping chunks that are sampled as independent utterances (own noise stream, own blind operator / RIR estimate) and
cross-faded back with linear ramps over the overlaps (a partition of unity: chunking the identity returns the input exactly)."""
from __future__ import annotations

import math

import torch


def chunk_plan(L, chunk, overlap):
    """equal-length chunks covering [0, L): starts (first 0, last L - chunk) spaced so that neighbours overlap by >= ``overlap`` samples"""
    if L <= chunk:
        return [0], L
    assert 0 <= overlap < chunk, "overlap must be smaller than the chunk"
    n = max(2, math.ceil((L - overlap) / (chunk - overlap)))
    return [round(i * (L - chunk) / (n - 1)) for i in range(n)], chunk


def pool_plan(lengths, chunk, overlap, batch_size):
    """Batches for a set of recordings of different lengths (``Tester.test_real_recordings``).  A file of at least ``chunk`` samples is cut with
    ``chunk_plan`` (equal chunks of ``chunk`` samples, never padded); the chunks of ALL such files form one pool that is cut, in file-then-chunk
    order, into batches of ``batch_size`` (the last may be smaller).  A shorter file is one chunk of its own length; such files share a batch only
    at exactly equal length, as ``Tester.test_dereverberation`` groups utterances.

    Returns ``(cuts, batches)``: ``cuts[f] = (starts, clen)`` and ``batches`` = lists of ``(f, k)`` (file, chunk number), every batch of one length."""
    batch_size = max(1, int(batch_size))
    cuts = [chunk_plan(int(L), chunk, overlap) for L in lengths]
    pool = [(f, k) for f, L in enumerate(lengths) if L >= chunk for k in range(len(cuts[f][0]))]
    batches = [pool[i:i + batch_size] for i in range(0, len(pool), batch_size)]
    short = {}
    for f, L in enumerate(lengths):
        if L < chunk:
            short.setdefault(int(L), []).append((f, 0))
    for grp in short.values():
        batches += [grp[i:i + batch_size] for i in range(0, len(grp), batch_size)]
    return cuts, batches


def run_bounds(n, max_rows):
    """``n`` chunks of one file as consecutive runs of at most ``max_rows`` chunks, near-equal in size: [(lo, hi), ...] (one run when they fit)"""
    max_rows = max(1, int(max_rows))
    r = max(1, math.ceil(n / max_rows))
    base, extra = divmod(n, r)
    out, lo = [], 0
    for j in range(r):
        hi = lo + base + (1 if j < extra else 0)
        out.append((lo, hi)); lo = hi
    return out


def pool_plan_shared(lengths, chunk, overlap, batch_size, max_rows):
    """``pool_plan`` for one RIR estimate per file (``real_recordings.shared_rir``): same cuts, same return shape, but a batch never splits a file,
    because a group of tied operator rows lives inside one operator.  Files are taken in order; a batch closes when the next file's chunks would
    take it past ``batch_size`` rows.  A file of more than ``batch_size`` chunks gets a batch of its own with all its chunks -- the batch, and the
    memory it takes, is then as large as the file, up to ``max_rows`` rows.  A file of more than ``max_rows`` chunks is cut into consecutive runs
    (``run_bounds``); each run is placed like a file and is a group of its own.  Short files as in ``pool_plan``.  ``shared_groups`` gives a
    batch's group map."""
    batch_size = max(1, int(batch_size))
    cuts = [chunk_plan(int(L), chunk, overlap) for L in lengths]
    batches, cur = [], []
    for f, L in enumerate(lengths):
        if L < chunk:
            continue
        for lo, hi in run_bounds(len(cuts[f][0]), max_rows):
            if cur and len(cur) + hi - lo > batch_size:
                batches.append(cur); cur = []
            cur = cur + [(f, k) for k in range(lo, hi)]
    if cur:
        batches.append(cur)
    short = {}
    for f, L in enumerate(lengths):
        if L < chunk:
            short.setdefault(int(L), []).append((f, 0))
    for grp in short.values():
        batches += [grp[i:i + batch_size] for i in range(0, len(grp), batch_size)]
    return cuts, batches


def shared_groups(cuts, batch, max_rows):
    """group map of one batch of ``pool_plan_shared``: row b -> number of its (file, run) within the batch (starts at 0, steps of 0 or 1)"""
    run_of = lambda f, k: next(j for j, (lo, hi) in enumerate(run_bounds(len(cuts[f][0]), max_rows)) if lo <= k < hi)
    keys = [(f, run_of(f, k)) for f, k in batch]
    out, g = [], 0
    for b, key in enumerate(keys):
        g += 1 if b and key != keys[b - 1] else 0
        out.append(g)
    return out


def crossfade_weights(starts, chunk, L, device=None):
    """(n, chunk) weights: 1 in the interior, linear ramps over the overlap with each neighbour; columns sum to 1 at every sample"""
    n = len(starts)
    w = torch.ones(n, chunk, device=device)
    for i in range(n - 1):
        ov = starts[i] + chunk - starts[i + 1]
        assert ov >= 0, "chunks must not leave gaps"
        if ov == 0:                       # L an exact multiple of the chunk with overlap 0: neighbours abut, plain concatenation
            continue
        ramp = (torch.arange(ov, device=device, dtype=torch.float32) + 0.5) / ov
        w[i, chunk - ov:] *= 1.0 - ramp
        w[i + 1, :ov] *= ramp
    return w


def split(y, chunk, overlap):
    """y (L,) or (1, L) -> (chunks (n, chunk), starts)"""
    y = y.reshape(-1)
    starts, clen = chunk_plan(y.shape[-1], chunk, overlap)
    return torch.stack([y[s:s + clen] for s in starts]), starts


def merge(parts, starts, L):
    """overlap-add of (n, chunk) sampled chunks back to (L,)"""
    n, chunk = parts.shape
    if n == 1:
        return parts[0, :L]
    w = crossfade_weights(starts, chunk, L, device=parts.device)
    out = torch.zeros(L, device=parts.device, dtype=parts.dtype)
    for i, s in enumerate(starts):
        out[s:s + chunk] += w[i] * parts[i]
    return out


def chunk_gains(parts, y):
    """(n, 1) level-match gains of ``predict_chunked``: std(y_chunk) / std(y_clip)"""
    return parts.std(dim=1, keepdim=True) / (y.reshape(-1).std() + 1e-12)


def predict_chunked(sample_batch, y, chunk, overlap, level_match=False):
    """``sample_batch``: (n, chunk) reverberant chunks -> (n, chunk) estimates (one sampler call, chunks = utterances).

    ``level_match``: the blind configuration rescales every utterance's estimate to a fixed standard deviation
    (``constraint_speech_magnitude``, reference EulerHeunSamplerDPS.py:127-129) -- per CHUNK here, so a chunk that is mostly a pause would come
    back as loud as a chunk of running speech and the cross-fade would mix segments of different gains.  With ``level_match`` each chunk's
    estimate is scaled by std(y_chunk) / std(y_clip) (the observation's own level profile) before the merge, which restores one gain for the clip;
    what remains chunk-specific is the RIR estimate (one operator per chunk, unless the chunks are tied into one group: ``shared_rir``), see profiles/DESIGN_history_r01-r04.md section 5.  Residual bias: the gain profile is the
    OBSERVATION's, and reverberation fills pauses, so a pause comes back louder than in the clean signal (measured pause / speech level 0.107
    against 0.052 in the input of tests/test_hip_cli.py's clip).  Chunks are never padded (equal chunks, the last one starts at L - chunk), so
    every std is over valid samples."""
    parts, starts = split(y, chunk, overlap)
    est = sample_batch(parts)
    if level_match and parts.shape[0] > 1:
        est = est * chunk_gains(parts, y).to(est.dtype)
    return merge(est, starts, y.reshape(-1).shape[-1])
