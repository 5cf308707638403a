"""The single 7-point step and the fused pair on the device, launched directly per region, kernel form and StencilTune
(stencil7.hip, stencil7_mfma.hip, stencil7x2.hip): every cell of the region bitwise equal to the torch CPU oracle and
every other byte of the `next` allocation untouched. The cases and the table of what launches what are in
stencil7_cases.py; test_stencil7_regions.py runs the host backend's share."""
import pytest
import torch

import stencil7_cases as cases
from star_cases import SHAPES, sub_regions

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SUBS = sorted(sub_regions(cases.SUB_SIZE))


@pytest.fixture
def dev(st):
    return st.Backend.Device


@pytest.fixture(scope="module", autouse=True)
def _drop_domains():
    yield
    cases.drop_domains()


def shape_id(s):
    (x, y, z), zc = s
    return f"{x}x{y}x{z}" + (f"-zc{zc}" if zc else "")


# ---- group A: the single step ----
@pytest.mark.parametrize("inst", list(cases.INSTANCES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_single_shapes_astaroth_fp32(st, dev, shape, inst):
    cases.case_single_shape(st, dev, shape[0], shape[1], inst, "astaroth", F32)


@pytest.mark.parametrize("inst", list(cases.INSTANCES))
@pytest.mark.parametrize("kind,dtype", [("jacobi", F32), ("astaroth", F64), ("jacobi", F64)],
                         ids=["jacobi-f32", "astaroth-f64", "jacobi-f64"])
@pytest.mark.parametrize("shape", cases.GROUP_SHAPES, ids=shape_id)
def test_single_shapes_other_types(st, dev, shape, kind, dtype, inst):
    cases.case_single_shape(st, dev, shape[0], shape[1], inst, kind, dtype)


@pytest.mark.parametrize("inst", list(cases.INSTANCES))
@pytest.mark.parametrize("kind,dtype", [("astaroth", F32), ("jacobi", F64)], ids=["astaroth-f32", "jacobi-f64"])
def test_single_odd_parity(st, dev, kind, dtype, inst):
    cases.case_single_parity(st, dev, inst, kind, dtype)


@pytest.mark.parametrize("inst", list(cases.INSTANCES))
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", SUBS)
def test_single_sub_regions_fp32(st, dev, name, kind, inst):
    cases.case_single_sub_region(st, dev, name, inst, kind, F32)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", SUBS)
def test_single_sub_regions_fp64(st, dev, name, kind):
    cases.case_single_sub_region(st, dev, name, cases.DEFAULT, kind, F64)


@pytest.mark.parametrize("shape", cases.MFMA_SHAPES, ids=shape_id)
def test_mfma_shapes(st, dev, shape):
    cases.case_single_shape(st, dev, shape[0], shape[1], cases.MFMA, "jacobi", F32)


@pytest.mark.parametrize("name", SUBS)
def test_mfma_sub_regions(st, dev, name):
    cases.case_single_sub_region(st, dev, name, cases.MFMA, "jacobi", F32)


def test_mfma_odd_parity(st, dev):
    cases.case_single_parity(st, dev, cases.MFMA, "jacobi", F32, size=(65, 17, 8), zchunk=3)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("inst", [cases.DEFAULT, "v0-ty4", "v1-ty4", "v2-nw16", "v0-ty2-plain-stores"])
@pytest.mark.parametrize("layout", sorted(cases.LAYOUT_SIZES))
def test_single_layouts(st, dev, layout, inst, kind, dtype):
    cases.case_single_layout(st, dev, layout, inst, kind, dtype)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("layout", sorted(cases.LAYOUT_SIZES))
def test_single_layouts_sub_region(st, dev, layout, dtype):
    size = cases.LAYOUT_SIZES[layout]
    sub = ((3, 1, 2), (size[0] - 2, size[1] - 1, size[2] - 1))
    cases.case_single_layout(st, dev, layout, cases.DEFAULT, "jacobi", dtype, sub=sub)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("mask", range(1, 8))
@pytest.mark.parametrize("size,dtype", cases.WRAP_CASES, ids=["24-f32", "22-f32", "22-f64"])
def test_single_wrap(st, dev, size, dtype, mask, kind):
    got = cases.case_single_wrap(st, dev, size, dtype, mask, kind)
    assert got == ("refused" if (mask & 1) and size[0] == 22 and dtype == F32 else "ran")


REGION_SETS = ["shell1", "shell2", "shell3", "width7and8", "many9", "many17"]


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("padded", [True, False], ids=["shell-kernel", "unpadded-regions-kernel"])
@pytest.mark.parametrize("name", REGION_SETS)
def test_single_regions(st, dev, name, padded, kind, dtype):
    cases.case_single_regions(st, dev, name, kind, dtype, padded)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_single_regions_wrap6(st, dev, kind, dtype):
    cases.case_single_regions(st, dev, "wrap6_x_slabs", kind, dtype)


def test_single_refusals(st, dev):
    cases.case_single_refusals(st, dev)


# ---- group B: the fused pair ----
@pytest.mark.parametrize("sched", cases.PAIR_SCHEDS)
@pytest.mark.parametrize("shape", cases.PAIR_COLUMN_SHAPES, ids=shape_id)
def test_pair_column_astaroth_fp32(st, dev, shape, sched):
    cases.case_pair(st, dev, shape[0], F32, "astaroth", x2sched=sched, zchunk=shape[1])


@pytest.mark.parametrize("sched", cases.PAIR_SCHEDS)
@pytest.mark.parametrize("kind,dtype", [("jacobi", F32), ("astaroth", F64), ("jacobi", F64)],
                         ids=["jacobi-f32", "astaroth-f64", "jacobi-f64"])
@pytest.mark.parametrize("shape", cases.PAIR_GROUP_SHAPES + [((256, 9, 6), 0)], ids=shape_id)
def test_pair_column_other_types(st, dev, shape, kind, dtype, sched):
    """(256, 9, 6) in fp64 is one two-chunk column: the form follows from the widths (cases.pair_form)"""
    cases.case_pair(st, dev, shape[0], dtype, kind, x2sched=sched, zchunk=shape[1])


@pytest.mark.parametrize("xfast", [0, 1])
@pytest.mark.parametrize("sched", cases.PAIR_SCHEDS)
@pytest.mark.parametrize("kind,dtype", [("astaroth", F32), ("jacobi", F64)], ids=["astaroth-f32", "jacobi-f64"])
def test_pair_column_order(st, dev, kind, dtype, sched, xfast):
    """x = 513: three block columns in fp32, five in fp64, in both column orders"""
    cases.case_pair(st, dev, (513, 17, 6), dtype, kind, form="column", x2sched=sched, x2xfast=xfast)


@pytest.mark.parametrize("sched", cases.PAIR_SCHEDS)
@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("name", SUBS)
def test_pair_sub_regions(st, dev, name, kind, dtype, sched):
    cases.case_pair_sub_region(st, dev, name, dtype, kind, sched)


@pytest.mark.parametrize("c", cases.pair_row_cases(), ids=cases.row_case_id)
def test_pair_row_forms(st, dev, c):
    cases.case_pair_row(st, dev, c)


@pytest.mark.parametrize("early", [True, False], ids=["early", "late"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("c", cases.PAIR_COL2_CASES, ids=cases.col2_case_id)
def test_pair_col2(st, dev, c, kind, early):
    cases.case_pair_col2(st, dev, c, kind, early=early)


def test_pair_col2_x_major(st, dev):
    cases.case_pair_col2(st, dev, cases.PAIR_COL2_CASES[1], "jacobi", xfast=1)


@pytest.mark.parametrize("size,dtype,kind,kw", [
    ((24, 9, 17), F32, "astaroth", dict(zchunk=5)), ((24, 9, 17), F64, "jacobi", dict(x2sched=1)),
    ((512, 9, 17), F32, "jacobi", dict(wrap=7)), ((645, 9, 17), F32, "astaroth", dict(wrap=1, zchunk=5)),
    ((512, 9, 17), F32, "astaroth", dict(wrap=6, zchunk=5)),
], ids=["column-zc5", "column-f64", "row-wrap7", "ragged3-wrap1-zc5", "col2-wrap6-zc5"])
def test_pair_odd_parity(st, dev, size, dtype, kind, kw):
    cases.case_pair_parity(st, dev, size, dtype, kind, **kw)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("shrink", sorted(cases.EXTERIOR_SHRINKS))
@pytest.mark.parametrize("size,dtype", cases.EXTERIOR_CASES, ids=["40-f32", "38-f64"])
def test_pair_exterior(st, dev, size, dtype, shrink, kind):
    cases.case_pair_exterior(st, dev, size, dtype, kind, shrink)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("wrap", sorted(cases.EXTERIOR_WRAPS))
@pytest.mark.parametrize("size,dtype", cases.EXTERIOR_CASES, ids=["40-f32", "38-f64"])
def test_pair_exterior_wrap(st, dev, size, dtype, wrap, kind):
    cases.case_pair_exterior(st, dev, size, dtype, kind, cases.EXTERIOR_WRAPS[wrap], wrap=wrap)


@pytest.mark.parametrize("dtype", cases.DTYPES, ids=cases.dtype_id)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("wrap", [0, 7])
@pytest.mark.parametrize("n", [9, 17])
def test_pair_regions(st, dev, n, wrap, kind, dtype):
    cases.case_pair_regions(st, dev, n, dtype, kind, wrap)


def test_pair_refusals(st, dev):
    cases.case_pair_refusals(st, dev)
