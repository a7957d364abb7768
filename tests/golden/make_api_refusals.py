"""Generate tests/golden/api_refusals.json: the status code and the complete lsr_last_error() text of every
refusal case of tests/test_api_refusals_cpu.py.

Run on the build machine only, with the library whose refusals are the contract -- a build of the commit
before a change to the API layer's checks, not the code under test:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_api_refusals.py <path to that liblsr.so>

Every case is refused before any device work (dummy pointers, never dereferenced), so no GPU is needed.
The output is a plain data file: {case id: {"code": int, "message": str}}.
"""
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from langsplat_amd import _native  # noqa: E402
from tests import test_api_refusals_cpu as cases  # noqa: E402


def main(lib_path):
    got = cases.run_cases(_native.load(os.path.abspath(lib_path)))
    bad = {k: v for k, v in got.items() if v["code"] != 1 or not v["message"]}
    if bad:
        raise SystemExit(f"not refused as LSR_ERR_INVALID: {bad}")
    with open(os.path.join(OUT, "api_refusals.json"), "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(got), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
