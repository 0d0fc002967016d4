"""Record tests/golden/y4m_calls.json: what the four Y4M stream drivers of ``rrin_amd.convert`` do with the
recording host model and the cases of ``tests/test_y4mpipe_host.py`` -- every model call, the SHA-256 of the
output (or of the report), the return value and the log line.  Only the public functions are called, so the
file records whatever code is checked out; it was recorded at the last commit that had the drivers in
``convert.py``, and the current code must reproduce it unchanged:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_y4m_calls.py

No GPU and no reference are needed (unlike ``gen_golden.py``)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from tests.test_y4mpipe_host import record_all  # noqa: E402


def main():
    path = os.path.join(HERE, "y4m_calls.json")
    with open(path, "w") as f:
        json.dump(record_all(), f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
