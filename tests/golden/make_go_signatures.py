#!/usr/bin/env python3
"""Writes tests/golden/reference_go_signatures.json: the reference's API facts tests/test_go_shim_signatures_cpu.py checks the Go shim
against (data only — parameter and result TYPES of mcts.MCTS's methods and of agogo.Inferer, mcts.New's signature, and how often
agent.go / arena.go make the calls INTEGRATION.md's `searcher` interface is built from).  Parsed with the test's own signature parser.

    python tests/golden/make_go_signatures.py <checkout of gorgonia/agogo>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_go_shim_signatures_cpu import _types, iface, methods  # noqa: E402


# what agent.go / arena.go call on Agent.MCTS (INTEGRATION.md's `searcher`), plus the tree's read-outs
SEARCHER = ("SetGame", "Search", "Policies", "Reset", "Log", "Nodes", "ToDot")


def main(ref):
    tree = "".join(open(os.path.join(ref, "mcts", f)).read() for f in ("tree.go", "search.go", "graph.go", "release.go"))
    agent, arena = open(os.path.join(ref, "agent.go")).read(), open(os.path.join(ref, "arena.go")).read()
    new = re.search(r"^func New\(([^)]*)\)\s*(\S+)\s*\{", tree, re.M)
    out = {
        "_source": "gorgonia/agogo: mcts/{tree,search,graph,release}.go, datatypes.go, agent.go, arena.go (tests/golden/make_go_signatures.py)",
        "mcts_methods": {k: list(v) for k, v in sorted(methods(tree, ("*MCTS", "lumberjack")).items()) if k in SEARCHER},
        "mcts_new": [_types(new.group(1)), _types(new.group(2))],
        "inferer": {k: list(v) for k, v in iface(open(os.path.join(ref, "datatypes.go")).read(), "Inferer").items()},
        "agent_go": {"field MCTS *mcts.MCTS": len(re.findall(r"MCTS\s+\*mcts\.MCTS", agent)),
                     "a.MCTS.SetGame(g)": agent.count("a.MCTS.SetGame(g)"), "a.MCTS.Search(a.Player)": agent.count("a.MCTS.Search(a.Player)")},
        "arena_go": {c: arena.count(c) for c in ("mcts.New(", ".MCTS.Policies(a.game)", "a.A.MCTS.Reset()", "a.A.MCTS.Log()")},
    }
    with open(os.path.join(HERE, "reference_go_signatures.json"), "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1])
