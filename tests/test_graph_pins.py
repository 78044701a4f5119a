"""The graphs that ``source_forward.fuse_bn_act`` builds and the BatchNorm chains that the matching twin recognises, node for
node against tests/golden/graph_pins.json (recorded by tests/golden/make_golden_graphs.py before the graph passes were
reorganised): every setting a caller uses, on both tiny fixtures and on a model with the add patterns they lack.  And the
twin graphs themselves (``twin_graphs``, recorded before the construction moved to ``methods/twin_graph.py``): every way a
caller builds one, in eval and in train mode.  Host only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_graphs as mgg  # noqa: E402  (the recipe: records, writes nothing on import)


def test_graphs_and_chains_are_the_recorded_ones(tiny_basic, tiny_bottleneck):
    with open(mgg.PINS) as f:
        want = json.load(f)
    models = {"tiny_basic": tiny_basic.m1, "tiny_bottleneck": tiny_bottleneck.m1, "add_patterns": mgg.AddPatterns().eval()}
    twins = {"tiny_bottleneck": mgg.tiny_axes(tiny_bottleneck), "add_patterns": None}      # + in_place, the recipe's own
    got = json.loads(json.dumps(mgg.record(models, twins)))
    assert sorted(got["fuse_bn_act"]) == sorted(want["fuse_bn_act"]) and len(want["fuse_bn_act"]) == len(models) * len(mgg.SETTINGS)
    for key, nodes in want["fuse_bn_act"].items():
        assert nodes and got["fuse_bn_act"][key] == nodes, key
    assert sorted(got["twin_chains"]) == sorted(want["twin_chains"]) and len(want["twin_chains"]) == 2 * len(models)
    for key, rows in want["twin_chains"].items():
        assert rows[:-1] and got["twin_chains"][key]["chains"] == rows[:-1], key
        assert rows[-1] == ["absorbed"] + got["twin_chains"][key]["absorbed"], key
    # the patterns the extra model is for: an add without a ReLU ends a chain of the twin; x + x ends none; one add, one chain
    ends = {row[0]: row for row in want["twin_chains"]["add_patterns/eval"][:-1]}
    assert ends["add"] == ["add", "bn1", "add", None, "x"] and ends["bn2"] == ["bn2", "bn2", None, None, None]
    assert [row[2] for row in ends.values()].count("add_2") == 1
    assert sorted(got["twin_graphs"]) == sorted(want["twin_graphs"])
    assert len(want["twin_graphs"]) == (len(twins) + 1) * 2 * len(mgg.TWIN_CONFIGS) == 30
    for key, nodes in want["twin_graphs"].items():
        assert nodes and got["twin_graphs"][key] == nodes, key
