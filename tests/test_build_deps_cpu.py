"""fr_build_id() hashes build.DEPS: a header that a source includes and DEPS forgets would make the id blind to its edits."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    spec = importlib.util.spec_from_file_location("_fr_build_deps", os.path.join(ROOT, "fractal-renderer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_file_reachable_from_the_sources_is_in_deps():
    build = _build()
    deps = {os.path.normpath(os.path.join(build.CSRC, d)) for d in build.DEPS}
    todo, seen = [os.path.join(build.CSRC, s) for s in build.SOURCES], set()
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        assert path in deps, "%s is compiled into the library but missing from build.DEPS" % os.path.relpath(path, ROOT)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
            todo.append(os.path.join(os.path.dirname(path), inc))
    assert len(seen) > len(build.SOURCES)  # the walk did find headers
    assert deps == seen, "build.DEPS lists files no source includes: %s" % sorted(os.path.relpath(d, ROOT) for d in deps - seen)
    assert set(build.KERNEL_SOURCES) <= set(build.SOURCES)
