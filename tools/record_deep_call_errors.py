#!/usr/bin/env python3
"""Records tests/golden/<table>_call_errors.json: the code and the fr_last_error text of every invalid call in
tests/<table>_call_cases.py, as the library of a given checkout answers them.  It only records; the tests that compare are
tests/test_deep_call_errors_cpu.py, tests/test_ss_call_errors_cpu.py and tests/test_de_call_errors_cpu.py (the plain DE calls).
Run it on the commit whose behaviour is to be pinned, before changing the host code:

    python tools/record_deep_call_errors.py [--table deep|ss|de] [--tree CHECKOUT] [--commit ID]

The table (default: deep) is always this repository's; CHECKOUT (default: this repository) is where the BUILT library is loaded
from.  ID (default: git rev-parse HEAD of CHECKOUT) goes into the file's header.  Needs no device, and refuses to write a file
if any call was not refused with FR_ERR_INVALID_ARGUMENT or FR_ERR_BUFFER_TOO_SMALL — or, for a case of the table that is named
a no-op, answered with FR_OK (recorded without a text) — or if an unspoiled call of the table (base_calls, where it has them)
does not get as far as the missing device."""
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    tree = os.path.abspath(argv[argv.index("--tree") + 1]) if "--tree" in argv else HERE
    name = argv[argv.index("--table") + 1] if "--table" in argv else "deep"
    commit = (argv[argv.index("--commit") + 1] if "--commit" in argv
              else subprocess.run(["git", "rev-parse", "HEAD"], cwd=tree, capture_output=True, text=True, check=True).stdout.strip())
    sys.path[:0] = [tree, os.path.join(HERE, "tests")]
    D = importlib.import_module(name + "_call_cases")
    from fractal_renderer_amd import _native

    assert os.path.dirname(_native.LIB_PATH) == os.path.join(tree, "fractal-renderer_amd"), _native.LIB_PATH
    lib, results, bad = _native.load(), {}, []
    for entry, fn, args, _keep in getattr(D, "base_calls", lambda _native: [])(_native):
        rc = getattr(lib, fn)(*args)
        if rc != (_native.FR_OK if "workspace" in fn else _native.FR_ERR_NO_DEVICE):
            bad.append("%s: the unspoiled call returned %d (%s)" % (entry, rc, lib.fr_last_error().decode()))
    made = 0
    for key, fn, args, *_keep in D.calls(_native):
        rc = getattr(lib, fn)(*args)
        made += 1
        if rc == _native.FR_OK and "noop_" in key:
            got = [rc, ""]
        elif rc in (_native.FR_ERR_INVALID_ARGUMENT, _native.FR_ERR_BUFFER_TOO_SMALL):
            got = [rc, lib.fr_last_error().decode()]
        else:
            bad.append("%s: returned %d, not a refusal" % (key, rc))
            continue
        if results.setdefault(key, got) != got:  # two calls of one id (a table may give a call and its twin one)
            bad.append("%s: %r from %s, %r before" % (key, got, fn, results[key]))
    if bad:
        sys.exit("\n".join(bad))
    out = {"header": "recorded by tools/record_deep_call_errors.py from the library of commit %s; each call: [code, fr_last_error]" % commit,
           "commit": commit}
    path = os.path.join(HERE, "tests", "golden", name + "_call_errors.json")
    with open(path, "w") as f:
        if hasattr(D, "pack"):  # a matrix (the table says how to read it), a row a line
            out.update(D.pack(results))
            rows = out.pop("rows")
            f.write("{\n" + "".join("%s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in out.items() if k != "answers"))
            f.write('"answers": [\n' + ",\n".join(json.dumps(a) for a in out["answers"]) + '\n],\n"rows": {\n')
            f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(rows.items())) + "\n}}\n")
        else:
            out["calls"] = results
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print("%d calls, %d answers -> %s" % (made, len(results), path))


if __name__ == "__main__":
    main(sys.argv[1:])
