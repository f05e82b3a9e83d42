"""Seeded synthetic transcript sets: uniform iid bases, chunked seeding so that any
row range can be generated independently (each rank makes only its own shard, the CPU baseline
only a prefix)."""
import numpy as np

CHUNK = 10_000
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def synthetic_codes(seed, n_seqs, length, start=0):
    """uint8 [n_seqs, length] of base codes 0..3 for rows start .. start+n_seqs-1."""
    out = np.empty((n_seqs, length), dtype=np.uint8)
    row, filled = start, 0
    while filled < n_seqs:
        chunk = row // CHUNK
        first = chunk * CHUNK
        rng = np.random.default_rng(np.random.SeedSequence([seed, chunk]))
        block = rng.integers(0, 4, size=(CHUNK, length), dtype=np.uint8)
        take = min(CHUNK - (row - first), n_seqs - filled)
        out[filled:filled + take] = block[row - first:row - first + take]
        filled += take
        row += take
    return out


def synthetic_ascii(seed, n_seqs, length, start=0):
    """(blob uint8 [n_seqs*length] of ASCII A/C/G/T, offsets int64 [n_seqs+1])."""
    blob = LETTERS[synthetic_codes(seed, n_seqs, length, start)].reshape(-1)
    offsets = np.arange(n_seqs + 1, dtype=np.int64) * length
    return blob, offsets


def profile_seqs(seed, n_seqs, length, n_profiles=3, sharpness=0.6):
    """(sequences, profile of each): n_seqs strings over ACGT, sequence i drawn from profile i % n_profiles — a first-order
    Markov chain whose transition rows are Dirichlet(sharpness) draws, so the profiles have clearly different k-mer
    spectra (the planted groups of the community tests and of tools/leiden_bench.py)."""
    rng = np.random.default_rng(seed)
    trans = rng.dirichlet([sharpness] * 4, size=(n_profiles, 4))
    cum = np.cumsum(trans, axis=2)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs, which = [], []
    for i in range(n_seqs):
        p = i % n_profiles
        u = rng.random(length)
        codes = np.empty(length, dtype=np.int64)
        state = int(rng.integers(4))
        for t in range(length):
            state = min(int(np.searchsorted(cum[p, state], u[t])), 3)
            codes[t] = state
        seqs.append(letters[codes].tobytes().decode("ascii"))
        which.append(p)
    return seqs, np.asarray(which)
