"""What StencilModel::init() decides, pinned as a whole: for a table of model configurations, every decision accessor
after init(), and again after each call of a fixed set_overlap_mode / set_overlap sequence (or that the call raised).
The result tests assert what a model computes; a model that quietly chose another, slower mode would pass them.

No case runs a step. Sizes are (x, y, z).

The expected values are tests/golden/model_decisions.json, recorded by running this module itself
(``python tests/test_gpu_model_decisions.py > tests/golden/model_decisions.json``) on a build of the commit named in the
file's header. They depend on the GPU (its resident blocks decide stencil7x2_row_kernel_used, hence can_pipeline) and on
the transports available to one process: the file is valid for one MI355X, the machine this suite runs on.

Which case reaches which stage of init():
  forwarding            forward-* (on; forward-pairs: pairs then stay off); every other case has it off
  pairs possible        pairs-*, triples-*-astaroth, jacobi-*, ranks2-pairs-* / ranks2-triples-* (on);
                        pairs-spheres-at-face and the thin triples-*-jacobi shapes (sphere margin: off); single-*
  pair overlap          pairs-1gpu / pairs-2dom (auto: no remote halo, off), pairs-forced-split (get_interior),
                        pairs-fake1 (an x face remote: off), pairs-fake4 / pairs-fake6 / triples-fake4 and the ranks2
                        cases (remote halos: local interior, comm reserve), pairs-fake*-mode2 (slabs after)
  pair wrap axes        pairs-* (wrap 7 / 3 / 1 / 0), pairs-forced-split (every wrapped axis cut), triples-512 (7),
                        triples-512-nowrap (0), triples-1024 / triples-256-fp64 (XH: 6), triples-645 (the ragged
                        exception keeps pairs), triples-645-nowrap, triples-645-2dom-xcut, triples-510-nowrap (refused)
  toggling, pipelining  one sub-domain whose z faces only count as remote (pairs-fake4-*) wraps z when whole and not
                        when overlapped: no toggle; pairs-fake4-2dom toggles (two sub-domains: no pipelining);
                        ranks2-pairs-zcut / -mode3 (pipelined pairs, from the start) and ranks2-triples-zcut (pipelined
                        triples) reach the publication counter; ranks2-pairs-ycut, ranks2-triples-xcut and
                        ranks2-triples-zcut-jacobi toggle without pipelining; the sequence walks every mode
  single-step plan      single-1gpu (wrap 7), single-nowrap, single-2dom (auto overlap off), single-2dom-forced /
                        single-1gpu-forced (classic split, confined translate), single-fake4 / ranks2-single (local
                        interior steps), single-fake4-classic / ranks2-single-classic, single-mfma*
  triples               triples-* (supported / refused), jacobi-pair-margin-only (pair margin passes, triple margin
                        fails), jacobi-triple-margin* (both pass), triples-fake4 / ranks2-triples-* (possible, but
                        overlapped by default: set_overlap_mode(0) / (4) turn them on)
  graphs, streams       every case
"""
import json
import os
import sys

import pytest

from conftest import run_ranks

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_decisions.json")

ACCESSORS = ("forwarding", "temporal_blocking", "temporal_triples", "overlapping", "overlap_mode", "can_toggle_overlap",
             "can_pipeline", "can_pipeline_triples", "local_interior_steps", "wrap_axes", "step_wrap_axes",
             "comm_reserve")

SEQUENCE = (("set_overlap_mode", 0), ("set_overlap_mode", 4), ("set_overlap_mode", 3), ("set_overlap_mode", 2),
            ("set_overlap_mode", 1), ("set_overlap", False), ("set_overlap", True))

MFMA = 8  # StencilTune::kMfma


def _case(name, kind, size, gpus=(0,), seq=False, **kw):
    return {"name": name, "kind": kind, "size": size, "gpus": list(gpus), "seq": seq, "kw": kw}


def _cases():
    out = [
        # single steps
        _case("single-1gpu", "jacobi", (48, 40, 36)),
        _case("single-nowrap", "jacobi", (48, 40, 36), wrap_self=False),
        _case("single-2dom", "jacobi", (48, 40, 36), (0, 0)),
        _case("single-2dom-forced", "jacobi", (48, 40, 36), (0, 0), overlap=True, auto_overlap=False),
        _case("single-1gpu-forced", "jacobi", (48, 40, 36), overlap=True, auto_overlap=False),
        _case("single-no-overlap", "jacobi", (48, 40, 36), (0, 0), overlap=False),
        _case("single-fake4", "jacobi", (48, 40, 36), seq=True, fake=4),
        _case("single-fake4-classic", "jacobi", (48, 40, 36), seq=True, fake=4, local_interior=False),
        _case("single-fake4-2dom", "jacobi", (48, 40, 36), (0, 0), seq=True, fake=4),
        _case("single-mfma", "jacobi", (48, 40, 36), variant=MFMA),
        _case("single-mfma-fake4", "jacobi", (48, 40, 36), seq=True, fake=4, variant=MFMA),
        _case("single-astaroth", "astaroth", (48, 40, 36)),
        # forwarding
        _case("forward-1gpu", "jacobi", (48, 40, 36), forward=True),
        _case("forward-2dom", "jacobi", (48, 40, 36), (0, 0), forward=True),
        _case("forward-pairs", "jacobi", (48, 40, 36), forward=True, temporal=2),
        # pairs
        _case("pairs-1gpu", "jacobi", (48, 40, 36), temporal=2),
        _case("pairs-2dom", "jacobi", (48, 40, 36), (0, 0), temporal=2),
        _case("pairs-fp64", "jacobi", (48, 40, 36), temporal=2, fp64=True),
        _case("pairs-nowrap", "jacobi", (48, 40, 36), temporal=2, wrap_self=False),
        _case("pairs-spheres-at-face", "jacobi", (260, 20, 18), temporal=2),
        _case("pairs-forced-split", "jacobi", (48, 40, 36), temporal=2, overlap=True, auto_overlap=False),
        _case("pairs-no-overlap-fake4", "jacobi", (48, 40, 36), seq=True, temporal=2, overlap=False, fake=4),
        _case("pairs-fake1", "jacobi", (48, 40, 36), seq=True, temporal=2, fake=1),
    ]
    for fake in (4, 6):
        for mode in (1, 2, 3):
            out.append(_case(f"pairs-fake{fake}-mode{mode}", "jacobi", (512, 112, 120), seq=True, temporal=2,
                             axis_cost=(64, 3, 2), fake=fake, overlap_mode=mode))
    out.append(_case("pairs-fake4-2dom", "jacobi", (512, 112, 120), (0, 0), seq=True, temporal=2, axis_cost=(64, 3, 2),
                     fake=4))
    # triples: the thin shapes put the Jacobi spheres (radius x / 10) on the y / z faces, so Jacobi falls back to single
    # steps there and the Astaroth proxy (no spheres) reaches the triple decisions
    for kind in ("jacobi", "astaroth"):
        out += [
            _case(f"triples-512-{kind}", kind, (512, 24, 16), temporal=3),
            _case(f"triples-512-nowrap-{kind}", kind, (512, 24, 16), temporal=3, wrap_self=False),
            _case(f"triples-1024-{kind}", kind, (1024, 24, 16), temporal=3),
            _case(f"triples-256-fp64-{kind}", kind, (256, 24, 16), temporal=3, fp64=True),
            _case(f"triples-645-{kind}", kind, (645, 24, 16), temporal=3),
            _case(f"triples-645-nowrap-{kind}", kind, (645, 24, 16), temporal=3, wrap_self=False),
            _case(f"triples-510-nowrap-{kind}", kind, (510, 24, 16), temporal=3, wrap_self=False),
            _case(f"triples-fake4-{kind}", kind, (512, 112, 120), seq=True, temporal=3, fake=4),
            _case(f"triples-645-2dom-xcut-{kind}", kind, (645, 30, 20), (0, 0), temporal=3, axis_cost=(1, 4, 4)),
        ]
    out += [
        # spheres of radius 51 centred at y = 52 / 53: y - r = 1 passes the pairs' margin (>= 1) and fails the triples'
        # (>= 2); at y = 107 the centre 53 leaves 2 below and y + r = 104 <= 107 - 3 above, so both pass
        _case("jacobi-pair-margin-only", "jacobi", (512, 105, 112), temporal=3),
        _case("jacobi-triple-margin", "jacobi", (512, 107, 112), temporal=3),
        _case("jacobi-triple-margin-nowrap", "jacobi", (512, 107, 112), temporal=3, wrap_self=False),
        _case("triples-mode4-start", "astaroth", (512, 112, 120), seq=True, temporal=3, fake=4, overlap_mode=3),
    ]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _cases()

# Two ranks sharing the GPU over HIP IPC, one sub-domain each: the only layout in which one machine has truly remote
# halos beside axes that wrap in-kernel, so the only one that reaches overlap toggling with pipelining (modes 3 / 4)
RANK_CASES = [
    _case("ranks2-single", "jacobi", (48, 40, 36), seq=True),
    _case("ranks2-single-classic", "jacobi", (48, 40, 36), seq=True, local_interior=False),
    _case("ranks2-pairs-zcut", "astaroth", (512, 16, 300), seq=True, temporal=2),
    _case("ranks2-pairs-zcut-mode3", "astaroth", (512, 16, 300), seq=True, temporal=2, overlap_mode=3),
    _case("ranks2-pairs-ycut", "astaroth", (512, 264, 16), seq=True, temporal=2, axis_cost=(4, 2, 3)),
    _case("ranks2-triples-zcut", "astaroth", (512, 16, 300), seq=True, temporal=3),
    # despite its name the default cost rule cuts this one along x (4 * 112 * 240 < 2 * 512 * 112): XH triples, wrap 6
    _case("ranks2-triples-zcut-jacobi", "jacobi", (512, 112, 240), seq=True, temporal=3),
    _case("ranks2-triples-xcut", "astaroth", (1024, 36, 40), seq=True, temporal=3, axis_cost=(1, 4, 4)),
]


def _build(st, case, group=None):
    kw = dict(case["kw"])
    if group is not None:
        kw["group"] = group
    fake, variant = kw.pop("fake", 0), kw.pop("variant", None)
    if fake:
        tr = st.TransportOptions()
        tr.fake_remote_axes = fake
        kw["transport"] = tr
    if variant is not None:
        t = st.StencilTune()
        t.variant = variant
        kw["tune"] = t
    if case["kind"] == "astaroth":
        m = st.AstarothSim(case["size"], quantities=2, gpus=case["gpus"], **kw)
    else:
        m = st.Jacobi3D(case["size"], gpus=case["gpus"], **kw)
    m.init()
    return m


def _state(m):
    return [int(getattr(m, a)()) for a in ACCESSORS]


def decisions(st, case, group=None):
    m = _build(st, case, group)
    out = {"init": _state(m)}
    if case["seq"]:
        out["sequence"] = []
        for fn, arg in SEQUENCE:
            try:
                getattr(m, fn)(arg)
                out["sequence"].append([f"{fn}({arg})", _state(m)])
            except Exception:  # noqa: BLE001  (whatever the binding maps the native error to)
                out["sequence"].append([f"{fn}({arg})", "raised"])
    m.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["accessors"] == list(ACCESSORS)
    return g["cases"]


def rank_decisions():
    """[rank] -> {case name: decisions} of RANK_CASES, from two ranks running this file as their worker"""
    outs = run_ranks(2, os.path.abspath(__file__), ["--rank-worker"],
                     env_extra={"MP_DEVICE": "1", "STENCIL_WAIT_TIMEOUT": "20"}, timeout=120)
    got = []
    for rc, out in outs:
        assert rc == 0, out[-3000:]
        got.append(json.loads([ln for ln in out.splitlines() if ln.startswith("DECISIONS ")][-1][10:]))
    return got


def test_golden_covers_the_table(golden):
    assert sorted(golden) == sorted(c["name"] for c in CASES + RANK_CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_model_decisions(st, golden, case):
    got = decisions(st, case)
    print(case["name"], dict(zip(ACCESSORS, got["init"])), got.get("sequence"))
    assert got == golden[case["name"]], dict(zip(ACCESSORS, got["init"]))


def test_model_decisions_two_ranks(golden):
    for rank, got in enumerate(rank_decisions()):
        for c in RANK_CASES:
            print(rank, c["name"], dict(zip(ACCESSORS, got[c["name"]]["init"])), got[c["name"]].get("sequence"))
            assert got[c["name"]] == golden[c["name"]], (rank, c["name"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    import stencil2_amd

    if "--rank-worker" in sys.argv:
        group = stencil2_amd.init_process_group()
        print("DECISIONS " + json.dumps({c["name"]: decisions(stencil2_amd, c, group) for c in RANK_CASES}), flush=True)
        sys.exit(0)
    info = stencil2_amd.build_info_string()
    head = {"recorded_from_commit": info.split("git=")[1].split()[0], "build": info,
            "device": torch.cuda.get_device_name(0), "accessors": list(ACCESSORS)}
    rows = [f"  {json.dumps(c['name'])}: {json.dumps(decisions(stencil2_amd, c))}" for c in CASES]  # one case per line
    ranks = rank_decisions()
    assert ranks[0] == ranks[1], "the two ranks decide differently"
    rows += [f"  {json.dumps(c['name'])}: {json.dumps(ranks[0][c['name']])}" for c in RANK_CASES]
    print(json.dumps(head, indent=1)[:-2] + ',\n "cases": {\n' + ",\n".join(rows) + "\n }\n}")
