"""tools/valu_budget.py: the join of k_pool's static VALU counts per region with the region table of a COUNT render
(prt_get_region_stats).  tests/golden/valu_join_c4.json is a recorded input: the static counts of one build of the default
k_pool variant and the region table of one C4 frame, with the measured SQ_INSTS_VALU of that frame's launch.
"""
from __future__ import annotations

import importlib.util
import json
import os
import re

import pytest

from conftest import GOLDEN, ROOT


def _tool():
    spec = importlib.util.spec_from_file_location("valu_budget", os.path.join(ROOT, "tools", "valu_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_region_names_follow_the_header():
    from par_raytracer_amd import capi
    text = open(os.path.join(ROOT, "include", "prt.h")).read()
    names = re.findall(r"\bPRT_REGION_([A-Z_]+)\b\s*(?:=\s*0)?,", text)
    assert [n.lower() for n in names] == capi.REGION_NAMES
    assert capi.hip_lib().prt_get_region_stats(None, None, 0) == -1
    # every counter the join multiplies by is a region of the table
    assert {c[0] if isinstance(c, tuple) else c for c in _tool().TIMES_OF.values()} <= set(capi.REGION_NAMES)


def test_join_multiplies_every_region_and_drops_none():
    vb = _tool()
    static = {"entry": 100, "trace.node_step": 95, "trace.leaf_tri": 80, "shade.pass.hit": 200}
    table = {"wave": [10, 640], "node_step": [1000, 32000], "tri": [300, 3000], "shade_hit": [7, 400], "node_push": [900, 0]}
    rows, total, rest = vb.join(static, table, 200000.0)
    assert [r[0] for r in rows] == sorted(static)
    assert {r[0]: r[5] for r in rows} == {"entry": 1000.0, "trace.node_step": 95000.0, "trace.leaf_tri": 24000.0, "shade.pass.hit": 1400.0}
    assert total == 121400.0 and rest == 78600.0
    assert dict((r[0], r[4]) for r in rows)["trace.node_step"] == 32.0          # mean active lanes
    assert vb.join(static, table)[2] is None
    assert vb.join({"trace.node_step.push": 30}, table)[1] == pytest.approx(9000.0)   # three pushes, counted one by one
    with pytest.raises(KeyError):                                               # a region nobody counts is not dropped quietly
        vb.join({"somewhere.else": 5}, table)
    with pytest.raises(KeyError):
        vb.join({"trace.finish": 5}, table)                                     # ... nor one whose counter the table lacks


def test_join_of_the_recorded_c4_frame(capsys):
    vb = _tool()
    g = json.load(open(os.path.join(GOLDEN, "valu_join_c4.json")))
    rows, total, rest = vb.join(g["static"], g["regions"], g["measured_valu"])
    assert len(rows) == len(g["static"])
    for r in rows:
        c = vb.TIMES_OF[r[0]]
        c, scale = c if isinstance(c, tuple) else (c, 1.0)
        assert r[5] == pytest.approx(g["static"][r[0]] * g["regions"][c][0] * scale, rel=1e-12)
    assert total == pytest.approx(g["expected_sum"], rel=1e-12)
    assert rest == pytest.approx(g["measured_valu"] - g["expected_sum"], rel=1e-9)
    # the bookkeeping condition the table was recorded under: the regions' products sum to within 10 % of the measured count
    assert abs(rest) <= 0.10 * g["measured_valu"]
    vb.print_join(g["static"], g["regions"], g["measured_valu"])
    out = capsys.readouterr().out
    assert "not accounted (measured - sum)" in out and "trace.node_step" in out
