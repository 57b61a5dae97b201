"""Golden fixture of stts_set_option / stts_get_option's semantics (tests/golden/option_semantics.json), recorded
from a built libstts2.so of the commit BEFORE a change to the option code, never from the changed tree:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_options.py

Host-only calls (no GPU).  For every live STTS_OPT_* key of include/stts2.h it records the value a fresh library
holds (`initial`, read before anything is set) and, for every probe value, [rc of set, get afterwards]; the key
is put back to `initial` before each probe, so a refused set (STTS_EINVAL) reads back `initial`.  The retired keys
and an unknown one are probed the same way (nothing to put back: they are never accepted).
"""
from __future__ import annotations

import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "styletts2-lite_amd"))
os.environ.pop("STTS_OPTS", None)  # lib() applies it on load

PROBES = [-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 64, 65, 1 << 20]
INVALID_KEYS = [3, 9, 26, 28, 999]  # the retired keys and an unknown one


def header_keys():
    """{NAME: key} of every `#define STTS_OPT_NAME <integer>` in include/*.h."""
    out = {}
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        out.update({n: int(v) for n, v in re.findall(r"^\s*#\s*define\s+STTS_OPT_(\w+)\s+(\d+)\s*$", open(h).read(),
                                                     flags=re.M)})
    return out


def record(L):
    keys = header_keys()
    live = {name: {"key": key, "initial": L.stts_get_option(key)} for name, key in sorted(keys.items(), key=lambda kv: kv[1])}
    for row in live.values():
        row["results"] = []
        for v in PROBES:
            assert L.stts_set_option(row["key"], row["initial"]) == 0
            row["results"].append([L.stts_set_option(row["key"], v), L.stts_get_option(row["key"])])
        assert L.stts_set_option(row["key"], row["initial"]) == 0
    invalid = {str(k): [[L.stts_set_option(k, v), L.stts_get_option(k)] for v in PROBES] for k in INVALID_KEYS}
    return {"probes": PROBES, "live": live, "invalid": invalid}


def main():
    from stts2_mi355x import engine
    path = os.path.join(HERE, "option_semantics.json")
    rec = record(engine.lib())
    rows = lambda d: ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in d.items())  # noqa: E731
    with open(path, "w") as f:  # one line per key
        f.write('{\n "probes": %s,\n "live": {\n%s\n },\n "invalid": {\n%s\n }\n}\n'
                % (json.dumps(rec["probes"]), rows(rec["live"]), rows(rec["invalid"])))
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
