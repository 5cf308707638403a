"""The cases of test_gpu_copy_types.py on the host backend (memmove path): they pin the byte oracle itself, the shape
query and the layouts for every element size, so a failure of the GPU file points at the HIP copy kernel."""
import numpy as np
import pytest

import copy_types_cases as cases
from stencil2_amd.utils.testing import cell_bytes


@pytest.fixture
def host(st):
    return st.Backend.Host


def test_cell_bytes_pattern():
    """never the poison byte, every byte of a cell depends on the byte index, the quantity, the tag and each
    coordinate"""
    gz = np.arange(5).reshape(-1, 1, 1)
    gy = np.arange(6).reshape(1, -1, 1)
    gx = np.arange(7).reshape(1, 1, -1)
    a = cell_bytes(gz, gy, gx, 2, 24, 0)
    assert a.shape == (5, 6, 7, 24) and a.dtype == np.uint8 and a.max() <= 250
    assert np.array_equal(a, cell_bytes(gz, gy, gx, 2, 24, 0))
    # a prefix of a wider element is the narrower element: the hash depends on b alone, not on es
    assert np.array_equal(a[..., :3], cell_bytes(gz, gy, gx, 2, 3, 0))
    for other in (cell_bytes(gz, gy, gx, 3, 24, 0), cell_bytes(gz, gy, gx, 2, 24, 1), cell_bytes(gz + 1, gy, gx, 2, 24, 0),
                  cell_bytes(gz, gy + 1, gx, 2, 24, 0), cell_bytes(gz, gy, gx + 1, 2, 24, 0)):
        # 251 values per byte: about 1 in 251 bytes agree by chance, never most of them, never a whole 24-byte cell
        assert (other == a).mean() < 0.02 and not (other == a).all(axis=-1).any()
    # the two halves of an element differ, and so do the bytes within it (a rotated or half-moved element fails)
    assert (a[..., :12] == a[..., 12:]).mean() < 0.02
    assert (a[..., :-1] == a[..., 1:]).mean() < 0.02
    assert not (np.roll(a, 1, axis=-1) == a).all(axis=-1).any()


def test_copy_seg_shape_rule(st):
    """the shape query: widest unit that divides the row bytes, both addresses and all four strides; rows are items
    up to 4 units"""
    f = st._C.copy_seg_shape
    D = st.Dim3
    assert f(0, 48, 480, 256, 128, 1280, D(12, 5, 4), 4) == {"vec": 16, "row_units": 3, "ny": 5, "units": 60, "rows": True}
    assert f(0, 48, 480, 264, 128, 1280, D(12, 5, 4), 4)["vec"] == 8  # destination address
    assert f(4, 48, 480, 256, 128, 1280, D(12, 5, 4), 4)["vec"] == 4  # source address
    assert f(0, 48, 480, 256, 130, 1280, D(12, 5, 4), 4)["vec"] == 2  # a stride
    assert f(0, 48, 480, 256, 128, 1281, D(12, 5, 4), 4)["vec"] == 1
    assert f(0, 6, 30, 256, 246, 2460, D(1, 5, 4), 6) == {"vec": 2, "row_units": 3, "ny": 5, "units": 60, "rows": True}
    w = f(0, 80, 400, 256, 128, 1280, D(20, 5, 4), 4)
    assert (w["vec"], w["row_units"], w["rows"]) == (16, 5, False)
    assert f(0, 0, 0, 256, 128, 1280, D(0, 5, 4), 4)["units"] == 0


@pytest.mark.parametrize("es", cases.REGION_ES)
def test_region_sweep(st, host, es):
    cases.case_region_sweep(st, host, es)


def test_region_sweep_covers_every_instance(st, host):
    cases.case_region_coverage(st, host)


@pytest.mark.parametrize("es", [4, 1])
def test_region_small_entries(st, host, es):
    cases.case_small_entries(st, host, es)


@pytest.mark.parametrize("ext,rows", [((2, 70, 60), 4200), ((2, 60, 60), 3600)])
@pytest.mark.parametrize("es", [4, 1])
def test_region_default_entries(st, host, es, ext, rows):
    cases.case_default_entries(st, host, es, ext, rows)


@pytest.mark.parametrize("es", [4, 1])
def test_region_wide_four_items(st, host, es):
    cases.case_wide_four_items(st, host, es)


# the transports of the device file that the host backend has: translate within the process and staged
@pytest.mark.parametrize("method,gpus", [("Kernel", [0]), ("Kernel", [0, 0]), ("Staged", [0, 0]), ("Staged", [0, 0, 0]),
                                         ("All", [0, 0, 0])])
@pytest.mark.parametrize("rname", ["r1", "r3", "asym", "fec"])
def test_exchange_mixed_types(st, host, method, gpus, rname):
    cases.case_exchange(st, host, method, gpus, rname)


@pytest.mark.parametrize("size,gpus", cases.LAYOUT_DOMAINS)
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("rname", ["r1", "r3", "asym", "fec"])
def test_exchange_mixed_types_layouts(st, host, layout, size, gpus, rname):
    cases.case_layout(st, host, layout, size, gpus, rname)


@pytest.mark.parametrize("size,gpus", cases.LAYOUT_DOMAINS)
@pytest.mark.parametrize("rname", ["r1", "r3", "asym", "fec"])
def test_exchange_shared_halo_lines_small_types(st, host, size, gpus, rname):
    cases.case_shared_lines_active(st, host, size, gpus, rname)


def test_typed_views_match_bytes(st, host):
    cases.case_typed_views(st, host)


def test_oracle_counts_wrong_cells(st, host):
    """the oracle is not vacuous: an exchange that is skipped, one flipped byte in a halo cell, one in the interior
    and a pattern of the wrong tag are all counted"""
    from stencil2_amd.utils.testing import check_exchange_bytes, fill_bytes_pattern
    radius = cases.radii(st)["fec"]
    dd, qs = cases.mixed_domain(st, host, (19, 13, 11), radius, [0], "Kernel")
    for q in qs:
        fill_bytes_pattern(dd, q, 0)
    d = dd.domain(0)
    raw = d.raw_size()
    halo_cells = raw.flatten() - d.size().flatten()  # fec (2, 1, 1): every direction has a radius
    assert all(check_exchange_bytes(dd, q, radius, 0) == halo_cells for q in qs)
    dd.exchange()
    assert all(check_exchange_bytes(dd, q, radius, 0) == 0 for q in qs)
    # another tag: a 1-byte cell agrees by chance once in 251, a wider one practically never
    assert all(check_exchange_bytes(dd, q, radius, 1) > 0.98 * raw.flatten() for q in qs)
    assert all(check_exchange_bytes(dd, q, radius, 1) == raw.flatten() for q in qs if d.elem_size(q) >= 6)
    for q in qs:
        es = d.elem_size(q)
        for pos in ((0, 0, 0), (5, 5, 5)):
            cell = bytearray(d.region_to_host(st.Dim3(*pos), st.Dim3(1, 1, 1), q, True))
            cell[es - 1] ^= 1
            d.region_from_host(st.Dim3(*pos), st.Dim3(1, 1, 1), q, bytes(cell), True)
        assert check_exchange_bytes(dd, q, radius, 0) == 2
