"""CPU: the inputs of tests/voxel_cases.py still meet the conditions they are named
for -- proved from the f2 oracle (oracle/voxel_oracle.cpp) and numpy alone, so an
edit to a seed or a size cannot quietly turn a case back into an easy one -- and on
every one of them the oracle's rows equal an independent numpy grouping's, order-free.
The GPU twin, test_voxel_edges_gpu.py, compares csrc/voxel.hip with the oracle byte
for byte on the same inputs."""
import numpy as np
import pytest

import voxel_cases as vc


# ---- each case meets the condition it is named for ---------------------------

def _lattice_sides(voxel, base):
    """Of the 1800 non-anchor quotients: (exactly integral, rounded just below an
    integer -- floor(q) < round(q), the lower cell --, rounded just above)."""
    pts, = vc.get(vc.lattice_name(voxel, base)).clouds
    assert pts.shape == (601, 3) and np.array_equal(pts.min(0), np.full(3, float(base)))
    q = vc.quotients(pts, voxel)[1:]
    assert np.abs(q - np.round(q)).max() < 1e-9          # nominally all on a face
    return int((q == np.round(q)).sum()), int((np.floor(q) < np.round(q)).sum()), int((q > np.round(q)).sum())


# (voxel, base) whose roundings all go one way: the products (g + 0.5) * voxel and
# the sums with these bases never come out an ulp short, so no quotient lies below
# its integer (figures printed by the test: 0.05 / -7.3 has 180 integral, 0 below,
# 1620 above).  They still have points exactly on a face and points an ulp off it.
LATTICE_ONE_SIDED = {(0.05, -7.3), (0.05, 1234.5), (1.0 / 3.0, 1234.5), (0.3, -7.3), (0.3, 1234.5)}


@pytest.mark.parametrize("base", vc.LATTICE_BASES)
@pytest.mark.parametrize("voxel", [v for v in vc.LATTICE_VOXELS if v != 1.0])
def test_lattice_quotients_sit_on_and_beside_cell_faces(oracle, voxel, base):
    on, below, above = _lattice_sides(voxel, base)
    rows = len(vc.oracle_case(oracle, vc.lattice_name(voxel, base))[0][0])
    print(f"voxel {voxel} base {base}: {on} integral, {below} just below, {above} just above, {rows} voxels")
    assert on >= 1                                        # exactly integral
    assert below + above >= 1                             # and an ulp off a face
    if (voxel, base) not in LATTICE_ONE_SIDED:
        assert below >= 1                                 # floor(q) < round(q): the lower cell
        assert rows < 601                                 # so nominal neighbours share a cell


@pytest.mark.parametrize("voxel", [v for v in vc.LATTICE_VOXELS if v != 1.0])
def test_lattice_every_voxel_size_straddles_both_ways(voxel):
    sides = [_lattice_sides(voxel, b) for b in vc.LATTICE_BASES]
    assert sum(s[0] for s in sides) >= 1 and sum(s[1] for s in sides) >= 1 and sum(s[2] for s in sides) >= 1


def test_lattice_counts_at_the_recorded_case(oracle):
    # all 1803 quotients, the anchor's three (0.5 each: "above") included
    q = vc.quotients(vc.get(vc.lattice_name(0.1, -7.3)).clouds[0], 0.1)
    r = np.round(q)
    assert ((q == r).sum(), (q < r).sum(), (q > r).sum()) == (345, 1015, 443)
    assert len(vc.oracle_case(oracle, vc.lattice_name(0.1, -7.3))[0][0]) == 216


@pytest.mark.parametrize("bits", vc.WIDE_SINGLE + (vc.WIDE_BATCH, vc.WIDE_TOO_FINE))
def test_wide_keys_have_the_requested_field_widths(oracle, bits):
    case = vc.get(vc.wide_name(bits))
    assert len(case.clouds) == (2 if bits == vc.WIDE_BATCH else 1)
    for pts, (rp, _, _) in zip(case.clouds, vc.oracle_case(oracle, vc.wide_name(bits))):
        assert len(pts) == 3500
        assert vc.key_bits(pts, case.voxel) == tuple(bits)
        # the oracle accepts every variant, the 65-bit one included (it returns -1,
        # raised as ValueError by oracle.py, only for the reference's own errors)
        assert 3000 <= len(rp) < 3500
        # the shifted copies: most share their original's voxel, a few were split off
        k = np.floor(vc.quotients(pts, case.voxel)).astype(np.int64)
        same = (k[:500] == k[3000:]).all(1)
        assert same.sum() >= 400 and (~same).sum() >= 3
    assert (sum(bits) + (1 if bits == vc.WIDE_BATCH else 0) > 64) == (bits == vc.WIDE_TOO_FINE)


def test_wide_keys_fill_the_sort_key(oracle):
    assert sum(vc.WIDE_SINGLE[0]) == 64 and sum(vc.WIDE_BATCH) + 1 == 64 and sum(vc.WIDE_TOO_FINE) == 65
    # unequal fields in both orders, so that swapped shifts or masks cannot cancel
    assert vc.WIDE_SINGLE[1][:2] == vc.WIDE_SINGLE[2][:2][::-1] and vc.WIDE_SINGLE[1][0] != vc.WIDE_SINGLE[1][1]


def test_threaded_replay_is_over_the_thread_threshold(oracle):
    case = vc.get("threaded")
    assert [len(c) for c in case.clouds] == [60000, 0, 60000]
    rows = [len(p) for p, _, _ in vc.oracle_case(oracle, "threaded")]
    print(f"threaded: voxels per cloud {rows}")
    assert sum(rows) >= 65536                              # V < 65536 stays serial
    assert sum(r > 0 for r in rows) >= 2                   # one cloud stays serial


def test_long_run_sum_depends_on_the_order():
    case = vc.get("long_run")
    pts, = case.clouds
    k = np.floor(vc.quotients(pts, case.voxel)).astype(np.int64)
    big = pts[(k == 11).all(1)]
    assert len(big) >= vc.LONG_RUN
    assert len(np.unique(k, axis=0)) > 1500               # among ordinary voxels
    seq, srt = np.zeros(3), np.zeros(3)
    for r in big:
        seq = seq + r
    for r in big[np.lexsort(big.T[::-1])]:
        srt = srt + r
    assert (seq != srt).all()                              # differs in bits on every axis
    # and the input order is no sorted order of the rows
    first = np.flatnonzero((k == 11).all(1))[:50]
    assert (np.diff(pts[first, 0]) < 0).any() and (np.diff(pts[first, 0]) > 0).any()


def test_layouts_hold_the_named_clouds(oracle):
    assert tuple(tuple(len(c) for c in vc.get(vc.layout_name(l)).clouds) for l in vc.LAYOUTS) == vc.LAYOUTS
    lens, b = vc.ONE_VOXEL
    case = vc.get(vc.layout_name(lens))
    assert vc.key_bits(case.clouds[b], case.voxel) == (0, 0, 0)
    rp, rn, rc = vc.oracle_case(oracle, vc.layout_name(lens))[b]
    assert rp.shape == rn.shape == rc.shape == (1, 3)
    for l in vc.LAYOUTS:
        case = vc.get(vc.layout_name(l))
        nan_rows = sum(int(np.isnan(n).any(1).sum()) for n in case.normals)
        comps = np.concatenate([np.flatnonzero(np.isnan(n).any(0)) for n in case.normals])
        # about 1/7 of the rows, never a whole row, all three components in turn
        assert abs(nan_rows - sum(l) / 7.0) <= len(l)
        assert all(not np.isnan(n).all(1).any() for n in case.normals)
        assert set(comps) == {0, 1, 2}
        # the other clouds are ordinary: many voxels, the larger ones with shared voxels
        for b, (c, (p, _, _)) in enumerate(zip(case.clouds, vc.oracle_case(oracle, vc.layout_name(l)))):
            if len(c) >= 40 and (l, b) != vc.ONE_VOXEL:
                assert len(c) // 4 < len(p) <= len(c)
            if len(c) >= 300:
                assert len(p) < len(c)


# ---- the oracle against the independent grouping -----------------------------

@pytest.mark.parametrize("name", list(vc.CASES))
def test_oracle_rows_equal_numpy_grouping(oracle, name):
    case = vc.get(name)
    for b, (pts, (rp, rn, rc)) in enumerate(zip(case.clouds, vc.oracle_case(oracle, name))):
        if not len(pts):
            assert rp.shape == (0, 3)
            continue
        nr = case.normals[b] if case.normals else None
        cl = case.colors[b] if case.colors else None
        ref = [a for a in (rp, rn, rc) if a is not None]
        got = vc._numpy_groups(pts, case.voxel, nr, cl)
        got = [got] if nr is None and cl is None else [a for a in got if a is not None]
        assert len(ref) == len(got)
        # whole rows (point | normal | color) sorted together: the extras of a voxel
        # must belong to that voxel's point
        assert np.array_equal(vc.sorted_rows(np.concatenate(ref, 1)), vc.sorted_rows(np.concatenate(got, 1)))
