"""Golden copy of the reference's shipped configuration tree, as data: every `configs/**/*.yml` of a reference checkout,
parsed with yaml.safe_load and stored under its path relative to `configs/` (one file per line).  The tests write the
entries back out as YAML files in the same layout -- the `../configs/...` indirections between them resolve as they do
in the checkout -- and build every object graph from them.  Run from the repo root:
    python tests/golden/make_golden_configs.py <path of a reference checkout>
"""
import glob
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_configs.json")


def main(ref: str) -> None:
    root = os.path.join(ref, "configs")
    paths = sorted(glob.glob(os.path.join(root, "**", "*.yml"), recursive=True))
    assert paths, f"no configs under {root}"
    entries = {}
    for p in paths:
        with open(p) as f:
            entries[os.path.relpath(p, root)] = yaml.safe_load(f)
    assert json.loads(json.dumps(entries)) == entries            # plain JSON data: string keys, no dates or tags
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True)}" for k, v in entries.items()) + "\n}\n")
    print(f"{OUT}: {len(entries)} configs")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
