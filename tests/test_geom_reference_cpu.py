"""The restatements of tests/geom_reference.py checked on their own, without a GPU: on a plane of dyadic points the normal stencil gives
the plane's normal, facing the camera; and each wrong variant — swapped du and dv, a missing orientation flip, a one-sided difference
where a central one is due, ``>`` for ``>=`` on acc_min, a median index off by one — is SEEN by the comparison the GPU tests use (bits
for the normals, the window rule for the median).  A comparison that cannot tell these apart would prove nothing there."""
import numpy as np
import pytest

import geom_reference as ref


def plane(H=6, W=7):
    """Points of the plane x + 2 y + 2 z = 4 with dyadic coordinates (every difference and product below is exact in fp32), seen from the
    side its normal (1,2,2)/3 points to; column step (2,-1,0)/4 x row step (0,1,-1)/4 = (1,2,2)/16."""
    r, c = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    P = np.stack([0.5 * c, 1.0 - 0.25 * c + 0.25 * r, 1.0 - 0.25 * r], -1).astype(np.float32)
    assert np.all(P[..., 0] + 2 * P[..., 1] + 2 * P[..., 2] == 4.0)
    cam = np.float32([8.0, 16.0, 16.0])
    return P, (P - cam).astype(np.float32)


def test_a_dyadic_plane_gives_its_normal_facing_the_camera():
    P, D = plane()
    acc = np.ones(P.shape[:2], np.float32)
    N, V = ref.point_normals(P, acc, D, 0.5)
    assert V.all()
    # |(1,2,2)/16| = 3/16 exactly, so every normal is (1,2,2)/3 rounded once per component — central, forward and backward differences alike
    want = (np.float32([1, 2, 2]) / np.float32(3)).astype(np.float32)
    assert ref.same_bits(N, np.broadcast_to(want, N.shape).copy())
    assert np.all((N * D).sum(-1) < 0)                                  # facing the camera
    behind = -D                                                       # the camera on the other side: the same plane, the opposite normal
    N2, V2 = ref.point_normals(P, acc, behind, 0.5)
    assert V2.all() and ref.same_bits(N2, -N)


def test_unusable_pixels_narrow_the_stencil_and_lonely_pixels_are_invalid():
    P, D = plane(5, 5)
    P = P.copy()
    P[2, 2] += np.float32(64.0)                                       # a point off the plane: whoever reads it gets another normal
    acc = np.ones((5, 5), np.float32)
    N, V = ref.point_normals(P, acc, D, 0.5)
    flat = (np.float32([1, 2, 2]) / np.float32(3)).astype(np.float32)
    reads = {(2, 1), (2, 3), (1, 2), (3, 2)}                          # its four neighbours, through their central differences
    for r in range(5):
        for c in range(5):
            assert ref.same_bits(N[r, c], flat) == ((r, c) not in reads), (r, c)
    acc[2, 2] = 0.25                                                  # unusable: nobody reads it, it is invalid itself
    N, V = ref.point_normals(P, acc, D, 0.5)
    assert V[2, 2] == 0 and not N[2, 2].any() and V.sum() == 24
    assert all(ref.same_bits(N[r, c], flat) for r in range(5) for c in range(5) if (r, c) != (2, 2))
    acc[:] = 0.0
    acc[1, 1] = acc[3, 3] = acc[3, 4] = 1.0                            # no usable neighbour / none along the rows
    N, V = ref.point_normals(P, acc, D, 0.5)
    assert not V.any() and not N.any()
    for shape in ((1, 5), (5, 1), (1, 1)):                            # one row or one column: one of the two differences never exists
        Q, E = plane(*shape)
        N, V = ref.point_normals(Q, np.ones(shape, np.float32), E, 0.5)
        assert not V.any() and not N.any()
    acc = np.ones((5, 5), np.float32)
    acc[0, 0] = np.nan                                                # NaN is not usable
    assert ref.point_normals(P, acc, D, 0.5)[1][0, 0] == 0
    Q = np.zeros((3, 3, 3), np.float32)                               # coincident points: a zero-length cross product is invalid
    N, V = ref.point_normals(Q, np.ones((3, 3), np.float32), np.ones((3, 3, 3), np.float32), 0.5)
    assert not V.any() and not N.any()


def scene():
    """Random points, acc around acc_min with exact ties, one grazing ray (n . d = 0 exactly) on an axis-aligned patch."""
    rng = np.random.default_rng(5)
    H, W = 7, 9
    P = rng.normal(size=(H, W, 3)).astype(np.float32)
    D = rng.normal(size=(H, W, 3)).astype(np.float32)
    acc = rng.uniform(0.3, 0.8, (H, W)).astype(np.float32)
    acc[rng.uniform(size=(H, W)) < 0.15] = np.float32(0.5)            # exactly acc_min: usable under >=, not under >
    r, c = np.meshgrid(np.arange(3, dtype=np.float32), np.arange(3, dtype=np.float32), indexing="ij")
    P[:3, :3] = np.stack([c, r, np.zeros_like(c)], -1)                 # a patch of the plane z = 0: normal (0,0,+-1), two components exactly 0
    acc[:3, :3] = 1.0
    D[1, 1] = (1.0, 0.0, 0.0)                                         # grazing: s = 0, no flip whatever the sign of n
    D[0, 0] = (0.0, 0.0, 1.0)
    return P, acc, D


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_the_bit_comparison_sees_each_wrong_stencil(fault):
    P, acc, D = scene()
    N, V = ref.point_normals(P, acc, D, 0.5)
    assert 0 < V.sum() < V.size
    Nf, Vf = ref.point_normals(P, acc, D, 0.5, fault=fault)
    assert not (ref.same_bits(N, Nf) and ref.same_bits(V, Vf)), fault
    if fault == "swap":                # dv x du = -(du x dv) and the flip undoes it, except on a grazing ray and in the sign of a zero
        assert not ref.same_bits(N[1, 1], Nf[1, 1]) and np.array_equal(N[1, 1], -Nf[1, 1])
        assert np.array_equal(N[0, 0], Nf[0, 0]) and not ref.same_bits(N[0, 0], Nf[0, 0])
    if fault == "strict":
        assert Vf.sum() < V.sum()


def test_the_median_window_is_exact_on_dyadic_weights_and_sees_an_index_off_by_one():
    rng = np.random.default_rng(9)
    R, S = 64, 33
    k = rng.multinomial(1024, np.ones(S) / S, size=R)
    k[0] = 0                                                          # never reaches the threshold
    k[1] = 0
    k[1, 4], k[1, 9] = 512, 512                                       # reaches it exactly, at index 4
    w = (k / 1024.0).astype(np.float32)
    z = np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1)
    index, depth = ref.median_exact(w, z, 0.5)
    assert index[0] == -1 and depth[0] == z[0, -1] and index[1] == 4 and depth[1] == z[1, 4]
    slow = [next((i for i in range(S) if float(np.sum(w[r, :i + 1], dtype=np.float64)) >= 0.5), -1) for r in range(R)]
    assert index.tolist() == slow
    tie = (np.cumsum(k, -1) == 512).any(-1)                           # a prefix sum ON the threshold: the window cannot exclude the next index
    bad, ambiguous = ref.median_check(w, z, 0.5, index, depth)
    assert bad.size == 0 and tie[1] and ambiguous == tie.mean()       # otherwise eps is below the 1/1024 grid: one admissible answer per ray
    for shift in (1, -1):
        off = index.copy()
        off[2:] = np.clip(off[2:] + shift, 0, S - 1)
        moved = np.flatnonzero((off != index) & ~tie)
        bad, _ = ref.median_check(w, z, 0.5, off, z[np.arange(R), off])
        assert moved.size > R // 2 and set(moved) <= set(bad.tolist()), shift
    bad, _ = ref.median_check(w, z, 0.5, index, np.roll(depth, 1))    # the right index with another sample's depth
    assert bad.size >= R - 2
    miss = index.copy()
    miss[5] = -1                                                      # -1 where the threshold is reached
    assert 5 in ref.median_check(w, z, 0.5, miss, np.where(miss < 0, z[:, -1], depth))[0]
    hit = index.copy()
    hit[0] = S - 1                                                    # an index where it never is
    assert 0 in ref.median_check(w, z, 0.5, hit, np.where(np.arange(R) == 0, z[:, -1], depth))[0]
    nan = w.copy()
    nan[3, 0] = np.nan
    assert ref.median_exact(nan, z, 0.5)[0][3] == -1
    late = w.copy()
    late[3, S - 1] = np.nan                                           # a NaN behind the crossing changes nothing
    assert ref.median_exact(late, z, 0.5)[0][3] == index[3]
    assert np.array_equal(ref.median_exact(w, z[0], 0.5)[1], z[0][np.where(index < 0, S - 1, index)])      # one shared row of depths


def test_the_window_is_narrow_on_composited_weights():
    """What the GPU test relies on: with alpha-compositing weights of random densities nearly every ray admits exactly one index, so the
    window rule pins the kernel's answer (measured here: 0 at S <= 65, at most 0.15 % at 192, 257, 600)."""
    rng = np.random.default_rng(11)
    for S in (65, 192, 600):
        sigma = np.maximum(rng.normal(size=(4096, S)), 0.0) * rng.uniform(0.0, 3.0, (4096, 1))
        w = ref.composite_weights(sigma, 0.1)
        z = np.linspace(8.0, 26.0, S, dtype=np.float32)
        index, depth = ref.median_exact(w, z, 0.5)
        bad, ambiguous = ref.median_check(w, z, 0.5, index, depth)
        assert bad.size == 0 and ambiguous <= 0.01, (S, ambiguous)
        assert (index >= 0).mean() > 0.2 and (index < 0).mean() > 0.005, S
