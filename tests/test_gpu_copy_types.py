"""The device copy kernel (csrc/src/kernels/copy.hip) over every element size and kernel form, bitwise against a byte
pattern: region copies steered into all 25 (vector width, row width) instances and the work-table edges, exchanges of
nine quantities of element sizes 1..24 B through every transport, layout and the few-CU grid-stride form, the typed
DLPack views of the narrow dtypes, and the fused wait + copy + signal kernel between two ranks on one GPU.
test_copy_types.py runs the same cases on the host backend."""
import os

import pytest

import copy_types_cases as cases
from conftest import run_ranks

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(__file__), "mp_worker.py")
RADII = ["r1", "r3", "asym", "fec"]


@pytest.fixture
def dev(st):
    return st.Backend.Device


# ---- the kernel directly: one region copy = one segment of a chosen (vec, row width) ----
@pytest.mark.parametrize("es", cases.REGION_ES)
def test_region_sweep(st, dev, es):
    """x offsets 0..5 and x extents 1..9, 16, 17, 33 of a (ex, 5, 4) box in a (37, 9, 7) radius-2 domain"""
    cases.case_region_sweep(st, dev, es)


def test_region_sweep_covers_every_instance(st, dev):
    """with the device addresses and pitches, the sweep above runs all 25 (vec, row width) instances"""
    cases.case_region_coverage(st, dev)


@pytest.mark.parametrize("es", [4, 1])
def test_region_small_entries(st, dev, es):
    cases.case_small_entries(st, dev, es)


@pytest.mark.parametrize("ext,rows", [((2, 70, 60), 4200), ((2, 60, 60), 3600)])
@pytest.mark.parametrize("es", [4, 1])
def test_region_default_entries(st, dev, es, ext, rows):
    cases.case_default_entries(st, dev, es, ext, rows)


@pytest.mark.parametrize("es", [4, 1])
def test_region_wide_four_items(st, dev, es):
    cases.case_wide_four_items(st, dev, es)


# ---- exchanges: nine quantities of mixed element sizes in one plan ----
@pytest.mark.parametrize("method,gpus", [("Kernel", [0]), ("Kernel", [0, 0]), ("PeerCopy", [0, 0]),
                                         ("PeerCopyEngine", [0, 0]), ("PeerCopyEngine", [0, 0, 0]), ("Rccl", [0, 0]),
                                         ("Staged", [0, 0]), ("All", [0, 0, 0])])
@pytest.mark.parametrize("rname", RADII)
def test_exchange_mixed_types(st, dev, method, gpus, rname):
    cases.case_exchange(st, dev, method, gpus, rname)


@pytest.mark.parametrize("size,gpus", cases.LAYOUT_DOMAINS)
@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("rname", RADII)
def test_exchange_mixed_types_layouts(st, dev, layout, size, gpus, rname):
    cases.case_layout(st, dev, layout, size, gpus, rname)


@pytest.mark.parametrize("size,gpus", cases.LAYOUT_DOMAINS)
@pytest.mark.parametrize("rname", RADII)
def test_exchange_shared_halo_lines_small_types(st, dev, size, gpus, rname):
    cases.case_shared_lines_active(st, dev, size, gpus, rname)


@pytest.mark.parametrize("knob,method,gpus", [("comm", "Staged", [0, 0]), ("comm", "Rccl", [0, 0]),
                                              ("comm", "PeerCopyEngine", [0, 0]), ("translate", "Kernel", [0]),
                                              ("translate", "Kernel", [0, 0])])
@pytest.mark.parametrize("blocks", [1, 3])
def test_exchange_mixed_types_few_cu_form(st, dev, knob, method, gpus, blocks):
    """copy_plan_kernel_narrow: the pack / unpack kernels (set_comm_max_blocks) or the same-GPU translate
    (set_translate_max_blocks) on 1 or 3 blocks of four groups. The x faces of (8, 36, 30) have 1080 rows, more than
    one 1024-item entry; with one block each group walks dozens of entries by grid stride."""
    radius = cases.radii(st)["fec"]
    dd, qs = cases.mixed_domain(st, dev, (8, 36, 30), radius, gpus, method)
    if knob == "comm":
        dd.set_comm_max_blocks(blocks)
    else:
        dd.set_translate_max_blocks(blocks)
    cases.exchange_twice(dd, qs, radius)


def test_typed_views_match_bytes(st, dev):
    cases.case_typed_views(st, dev)


# ---- the fused wait + copy + signal kernel (Colocated transport): two ranks sharing GPU 0 ----
@pytest.mark.parametrize("variant", [{}, {"MP_COLO_COPY": "Engine"}, {"MP_FUSE_FLAGS": "0"}],
                         ids=["fused-store", "engine", "unfused"])
@pytest.mark.parametrize("radius", ["fec", "asym"])
def test_colocated_mixed_types_two_ranks(radius, variant):
    env = {"MP_DEVICE": "1", "MP_METHODS": "Colocated|Kernel", "STENCIL_WAIT_TIMEOUT": "20", **variant}
    for rc, out in run_ranks(2, WORKER, ["exchange_types", radius, "20,12,10"], env_extra=env):
        assert rc == 0, out[-3000:]
        assert "types bad 0" in out, out[-3000:]
