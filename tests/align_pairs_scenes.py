"""Scenes and references shared by the align_pairs tests (tests/test_align_pairs_gpu.py, tests/test_align_pairs_adapter.py): clouds are
synth.planar_pair(n=8192) and slices of it, every reference is today's per-target path -- setInputTarget(target) + setInputSource(source)
+ align(guess) + getFitnessScore() on a Registration of its own -- computed once per process and left unchanged."""
import numpy as np

from delta_graph_slam_amd import synth

DMAX = 2.0          # gicp_max_correspondence_distance of every registration here (tests/test_gicp_gpu.py's)
POSE_TOL = (1e-6, 1e-7)   # metres, radians: the project's batch-against-single figures (tests/test_gicp_gpu.py:138-142)
FIT_RTOL = 1e-9

# nn_group.h / nn_bvh.hip: an index leaf holds kLeaf = 8 points and a node has kFan = 8 children, so the tree gains a level past 64, 512 and
# 4,096 points.  gicp.hip, gicp_correspond_kernel: a wave walks 8 adjacent source points per round (8 lanes a point), a workgroup
# kBlock / 8 = 32, and a wave's stretch is 8 x run points with run = ceil(n / (32 x workgroups of the pair)).
K_LEAF, K_FAN, ROUND_POINTS, BLOCK_QUERIES = 8, 8, 8, 32

_CACHE = {}


def base():
    if "base" not in _CACHE:
        _CACHE["base"] = synth.planar_pair(n=8192)
    return _CACHE["base"]


def make_registration(cov_mode=0, **kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration("FAST_GICP", gicp_max_correspondence_distance=DMAX, gicp_cov_jacobi_svd=cov_mode, **kw)


def subset(cloud, m, seed):
    """m points of `cloud` drawn without order: every surface of the scene is in it (a leading slice of planar_pair is ground alone)"""
    return cloud[np.random.default_rng(seed).permutation(cloud.shape[0])[:m]].copy()


def near(cloud, center, k):
    """the k points of `cloud` nearest to `center`, in the cloud's own order"""
    d = np.linalg.norm(cloud[:, :3] - np.asarray(center, np.float32)[None, :], axis=1)
    return cloud[np.sort(np.argsort(d, kind="stable")[:k])].copy()


def corner_clouds(n_target, n_source):
    """Small clouds around the corner where the ground and the two walls of the scene meet (all six degrees of freedom are held there):
    the n_target target points and the n_source source points nearest to it, the source in its own frame."""
    tgt, src, T = base()
    corner = np.array([9.0, 9.0, 0.5])
    Tinv = np.linalg.inv(T)
    return near(tgt, corner, n_target), near(src, Tinv[:3, :3] @ corner + Tinv[:3, 3], n_source)


def many_sources():
    """the 11 + 1 sources and guesses of test_gicp_gpu.py::test_batch_of_many_pairs_matches_single_aligns, the empty source included"""
    tgt, src, _ = base()
    rng = np.random.default_rng(5)
    sources, guesses = [], []
    for _ in range(11):
        m = int(rng.integers(500, 8192))
        sources.append(src[rng.permutation(8192)[:m]].copy())
        guesses.append(synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32))
    sources.insert(4, np.zeros((0, 4), np.float32))
    guesses.insert(4, np.eye(4, dtype=np.float32))
    return tgt, sources, guesses


def distinct_pairs():
    """3 targets of different sizes, 9 pairs interleaved A, B, C, A, ... and a tenth with a deliberately poor guess (it finishes many rounds
    after the others, so the workgroups are re-dealt across targets while it runs) -> (clouds, [(target, source, guess)]) by index"""
    if "distinct" in _CACHE:
        return _CACHE["distinct"]
    tgt, src, _ = base()
    rng = np.random.default_rng(11)
    clouds = [tgt, subset(tgt, 5000, 21), subset(tgt, 4500, 22)]
    pairs = []
    for k in range(9):
        m = int(rng.integers(500, 8192))
        clouds.append(src[rng.permutation(8192)[:m]].copy())
        pairs.append((k % 3, len(clouds) - 1, synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32)))
    pairs.append((1, 3 + 4, synth.make_transform((2.5, 2.0, 0.5), (0.1, -0.1, 0.8)).astype(np.float32)))
    _CACHE["distinct"] = (clouds, pairs)
    return _CACHE["distinct"]


def single_reference(clouds, pairs, cov_mode=0, key=None):
    """Today's path per pair on a Registration of its own: one dict per pair (T, converged, iterations, evaluations, status, fitness)."""
    if key is not None and (key, cov_mode) in _CACHE:
        return _CACHE[(key, cov_mode)]
    single = make_registration(cov_mode)
    out = []
    for t, s, g in pairs:
        if clouds[t].shape[0] == 0 or clouds[s].shape[0] == 0:
            out.append(None)
            continue
        single.setInputTarget(clouds[t])
        single.setInputSource(clouds[s])
        single.align(g)
        lr = single.last_result
        out.append(dict(T=single.getFinalTransformation(), converged=single.hasConverged(), iterations=lr.iterations, evaluations=lr.evaluations,
                        status=lr.status, fitness=single.getFitnessScore()))
    single.close()
    if key is not None:
        _CACHE[(key, cov_mode)] = out
    return out


def compare(res, ref, what=""):
    """One pair of align_pairs against today's path: equal flags and counts, pose within POSE_TOL (or the very bits: a degenerate pair may
    hold NaN on both sides), fitness within FIT_RTOL.  -> (translation difference, rotation difference, relative fitness difference)"""
    from tests.helpers import pose_error
    assert res["status"] == 0, (what, res["status"])
    assert res["converged"] == ref["converged"], what
    assert res["iterations"] == ref["iterations"] and res["evaluations"] == ref["evaluations"], (what, res["iterations"], ref["iterations"],
                                                                                                 res["evaluations"], ref["evaluations"])
    if np.array_equal(res["T"], ref["T"], equal_nan=True):
        dt = dr = 0.0
    else:
        dt, dr = pose_error(res["T"], ref["T"])
        assert dt <= POSE_TOL[0] and dr <= POSE_TOL[1], (what, dt, dr)
    if res["fitness"] == ref["fitness"] or (np.isnan(res["fitness"]) and np.isnan(ref["fitness"])):
        df = 0.0
    else:
        df = abs(res["fitness"] - ref["fitness"]) / abs(ref["fitness"])
        assert df <= FIT_RTOL, (what, res["fitness"], ref["fitness"])
    return dt, dr, df
