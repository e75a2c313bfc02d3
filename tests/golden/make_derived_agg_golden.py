#!/usr/bin/env python3
"""Generate tests/golden/derived_agg_reference.json: what the UNMODIFIED reference does with the plans of tests/derivedcases.py
(derived aggregations) over tpch_full.database(0.01) and the two literal tables, at one thread: its result text, or its refusal.
A result above 4 KB is stored as its SHA-256 and row count.

Run where the reference is built (oracle/_ref/ref_harness):  python tests/golden/make_derived_agg_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from resql_amd import tpch_full  # noqa: E402
from oracle import orc  # noqa: E402
import derivedcases as D  # noqa: E402

SF = 0.01
INLINE_BYTES = 4096


def main():
    db = tpch_full.database(SF)
    out = {"sf": SF, "cases": {}, "refused": {}}
    for f in D.CASES:
        text, _ = orc.run_reference(f(db), threads=1)
        case = {"rows": text.count("\n") - 1, "sha256": hashlib.sha256(text.encode()).hexdigest()}
        if len(text) <= INLINE_BYTES:
            case["text"] = text
        out["cases"][f.__name__] = case
        print(f.__name__, "->", case["rows"], "rows", file=sys.stderr)
    for f, _ in D.REFUSED:
        try:
            orc.run_reference(f(db), threads=1)
            raise SystemExit(f.__name__ + ": the reference answered")
        except orc.OracleError as e:
            lines = [l.strip() for l in str(e).strip().splitlines() if l.strip()]
            words = [l for l in lines if "what():" in l or l.startswith("ResqlError:")]
            out["refused"][f.__name__] = (words[0] if words else lines[-1])[:300]
        print(f.__name__, "->", out["refused"][f.__name__], file=sys.stderr)
    with open(os.path.join(HERE, "derived_agg_reference.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
