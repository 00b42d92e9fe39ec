#!/usr/bin/env python3
"""Records tests/golden/deep_call_errors.json: the code and the fr_last_error text of every invalid call in
tests/deep_call_cases.py, as the library of a given checkout answers them.  It only records; the test that compares is
tests/test_deep_call_errors_cpu.py.  Run it on the commit whose behaviour is to be pinned, before changing the host code:

    python tools/record_deep_call_errors.py [--tree CHECKOUT] [--commit ID]

CHECKOUT (default: this repository) is where the BUILT library is loaded from; the table of cases is always this
repository's.  ID (default: git rev-parse HEAD of CHECKOUT) goes into the file's header.  Needs no device, and refuses to
write a file if any call was not refused with FR_ERR_INVALID_ARGUMENT or FR_ERR_BUFFER_TOO_SMALL."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    tree = os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else HERE
    commit = (argv[argv.index("--commit") + 1] if "--commit" in argv
              else subprocess.run(["git", "rev-parse", "HEAD"], cwd=tree, capture_output=True, text=True, check=True).stdout.strip())
    sys.path[:0] = [tree, os.path.join(HERE, "tests")]
    import deep_call_cases as D
    from fractal_renderer_amd import _native

    assert os.path.dirname(_native.LIB_PATH) == os.path.join(tree, "fractal-renderer_amd"), _native.LIB_PATH
    lib, results = _native.load(), {}
    for key, fn, args, _keep in D.calls(_native):
        rc = getattr(lib, fn)(*args)
        if rc not in (_native.FR_ERR_INVALID_ARGUMENT, _native.FR_ERR_BUFFER_TOO_SMALL):
            sys.exit("%s: returned %d, not a refusal" % (key, rc))
        results[key] = [rc, lib.fr_last_error().decode()]
    out = {"header": "recorded by tools/record_deep_call_errors.py from the library of commit %s; each call: [code, fr_last_error]" % commit,
           "commit": commit, "calls": results}
    path = os.path.join(HERE, "tests", "golden", "deep_call_errors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d calls -> %s" % (len(results), path))


if __name__ == "__main__":
    main(sys.argv[1:])
