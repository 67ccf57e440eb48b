"""Inputs of fixture G12 (tests/golden/make_golden_width.py), rebuilt instead of stored: the frames come from seeded numpy
generators (the fixture keeps their SHA-256, so a changed generator stream fails loudly), and the large gradient tensors are kept
as fixed +-1 sketches."""
import hashlib

import numpy as np

SMALL = 4608            # tensors up to this many elements are stored whole (as make_golden.py's G4)
N_PROJ = 16             # sketch rows per large tensor


def frames_fwd():
    """8 frames for the forward check; frame 1 has flat colour regions (max-pool ties), frame 2 is black (as G3)."""
    obs = np.random.default_rng(7).integers(0, 256, size=(8, 64, 64, 3), dtype=np.uint8)
    obs[1, :, :32] = 17
    obs[1, :, 32:] = 200
    obs[2] = 0
    return obs


def frames_rollout(T=4, E=8):
    """The frames make_golden.synth_rollout draws first from default_rng(11)."""
    return np.random.default_rng(11).integers(0, 256, size=(T + 1, E, 64, 64, 3), dtype=np.uint8)


def frames_rec(E=8):
    """The recurrent prediction's three steps of frames: the first draw of default_rng(23)."""
    return np.random.default_rng(23).integers(0, 256, size=(3, E, 64, 64, 3), dtype=np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def signs(n):
    """(N_PROJ, n) rows of +-1 / sqrt(n) from an integer hash (no random generator): unit vectors, so for any tensors g, r
    |s . g - s . r| <= ||g - r||, and a bound on the relative L2 error bounds every sketch entry by the same fraction of ||r||."""
    j = np.arange(N_PROJ, dtype=np.uint64)[:, None]
    i = np.arange(n, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0x5bd1e995)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return np.where((h & np.uint64(1)) == 1, 1.0, -1.0) / np.sqrt(n)


def sketch(a):
    """-> (N_PROJ,) float64 projections of a (flattened, in float64)."""
    a = np.asarray(a, np.float64).ravel()
    return signs(a.size) @ a


def grad_errors(g, z, prefix="raw/"):
    """name -> error of gradient g[name] against fixture z, as a fraction of the reference's L2 norm.  Whole tensors: the relative L2
    error.  Large tensors: the worst of |norm - norm_ref|, |sum - sum_ref| / sqrt(n) and the sketch entries -- each is at most the
    relative L2 error, so a bound on these is implied by the same bound on the whole tensor.  That is a necessary condition only (an
    error spread over a large tensor moves its sketch far less than its L2 norm): tests/test_gpu_width.py also compares every tensor
    whole against the CPU oracle, which tests/test_width_host.py pins to this fixture."""
    out = {}
    for k in z.files:
        if k.startswith(prefix + "g/"):
            name = k[len(prefix) + 2:]
            r = z[k].astype(np.float64).ravel()
            out[name] = float(np.linalg.norm(np.asarray(g[name], np.float64).ravel() - r) / (np.linalg.norm(r) + 1e-12))
        elif k.startswith(prefix + "norm/"):
            name = k[len(prefix) + 5:]
            a = np.asarray(g[name], np.float64).ravel()
            nrm = float(z[k])
            errs = [abs(np.linalg.norm(a) - nrm), abs(a.sum() - float(z[prefix + "sum/" + name])) / np.sqrt(a.size),
                    float(np.abs(sketch(a) - z[prefix + "sketch/" + name]).max())]
            out[name] = max(errs) / (nrm + 1e-12)
    return out
