"""Where the Python layer creates device tensors, read from its source: no GPU.

A wrapper that takes ``stream=`` launches the library on that stream, so whatever it allocates, zero-fills or uploads has to be
ordered on that stream too: a ``torch.zeros`` on torch's current stream is unordered against a launch on a side stream, and lands
after it when the current stream is busy.  The decision is stated once, in ``psxavenc_amd/_lib.py`` (``launch_stream``,
``new_tensor``, ``to_device``); this test keeps every wrapper on it.
"""
import ast
import glob
import os

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "psxavenc_amd")
HELPERS = ("launch_stream", "new_tensor", "to_device")          # psxavenc_amd/_lib.py: the only functions exempt
FACTORIES = ("zeros", "empty", "full")                          # torch.<name>(...)
MOVES = ("to", "cuda")                                          # <tensor>.<name>(...)


def _modules():
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            yield os.path.basename(path), ast.parse(f.read(), path)


def _functions(tree):
    """(function node, the calls in its own body: those of nested functions belong to the nested function)"""
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            continue
        calls, todo = [], list(fn.body)
        while todo:
            node = todo.pop()
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                continue
            if isinstance(node, ast.Call):
                calls.append(node)
            todo.extend(ast.iter_child_nodes(node))
        yield fn, calls


def _params(fn):
    a = fn.args
    return [p.arg for p in a.posonlyargs + a.args + a.kwonlyargs]


def _dotted(node):
    parts = []
    while isinstance(node, ast.Attribute):
        parts.append(node.attr)
        node = node.value
    if isinstance(node, ast.Name):
        parts.append(node.id)
        return ".".join(reversed(parts))
    return None


def _is_helper(mod, fn):
    return mod == "_lib.py" and fn.name in HELPERS


def _scan():
    """the findings of one pass over the package: (direct factories, direct moves / current_stream in stream functions,
    helper calls that do not pass the function's stream, number of helper calls seen in stream functions)"""
    factories, direct, unbound, seen = [], [], [], 0
    for mod, tree in _modules():
        for fn, calls in _functions(tree):
            if _is_helper(mod, fn):
                continue
            takes_stream = "stream" in _params(fn)
            for c in calls:
                name = _dotted(c.func)
                where = "%s:%d %s" % (mod, c.lineno, fn.name)
                if name in tuple("torch." + f for f in FACTORIES):
                    factories.append(where + " " + name)
                if not takes_stream:
                    continue
                if isinstance(c.func, ast.Attribute) and c.func.attr in MOVES and name not in ("_lib.to_device",):
                    direct.append(where + " ." + c.func.attr + "(")
                if name == "torch.cuda.current_stream":
                    direct.append(where + " " + name)
                if name in tuple("_lib." + h for h in HELPERS):
                    seen += 1
                    first = c.args[0] if c.args else next((k.value for k in c.keywords if k.arg == "stream"), None)
                    if not (isinstance(first, ast.Name) and first.id == "stream"):
                        unbound.append(where + " " + name)
    return factories, direct, unbound, seen


@pytest.fixture(scope="module")
def scan():
    return _scan()


def test_the_helper_is_where_the_issue_says(scan):
    lib = dict(_modules())["_lib.py"]
    names = {fn.name for fn in ast.walk(lib) if isinstance(fn, ast.FunctionDef)}
    assert set(HELPERS) <= names
    for fn, calls in _functions(lib):
        if fn.name in ("new_tensor", "to_device"):
            # the allocation happens with the launch stream current: under `with torch.cuda.stream(launch_stream(stream, ...))`
            withs = [w for w in ast.walk(fn) if isinstance(w, ast.With)]
            assert len(withs) == 1 and _dotted(withs[0].items[0].context_expr.func) == "torch.cuda.stream"
            inner = withs[0].items[0].context_expr.args[0]
            assert _dotted(inner.func) == "launch_stream" and inner.args[0].id == "stream"
            made = [c for c in ast.walk(withs[0]) if isinstance(c, ast.Call) and
                    (_dotted(c.func) in tuple("torch." + f for f in FACTORIES) or (isinstance(c.func, ast.Attribute) and c.func.attr in MOVES))]
            outside = [c for c in calls if c not in list(ast.walk(withs[0])) and
                       (_dotted(c.func) in tuple("torch." + f for f in FACTORIES) or (isinstance(c.func, ast.Attribute) and c.func.attr in MOVES))]
            assert made and not outside, fn.name


def test_no_wrapper_creates_a_device_tensor_itself(scan):
    factories, _, _, _ = scan
    assert factories == [], "torch.zeros / torch.empty / torch.full outside _lib.new_tensor:\n" + "\n".join(factories)


def test_no_stream_function_moves_or_resolves_on_its_own(scan):
    _, direct, _, _ = scan
    assert direct == [], "a function that takes stream= resolves or uploads past the helper:\n" + "\n".join(direct)


def test_the_helper_gets_the_functions_stream(scan):
    _, _, unbound, seen = scan
    assert seen >= 40, "the scan found %d helper calls in functions that take stream=: it is not looking at the wrappers" % seen
    assert unbound == [], "helper called with something else than the function's `stream`:\n" + "\n".join(unbound)


def test_every_function_that_hands_a_stream_to_the_library_resolves_it_through_the_helper():
    """`.cuda_stream` is what reaches the C layer: in a function that takes stream=, it is read from launch_stream(stream, ...) --
    directly, through a local bound to it, or through the module's own one-line resolver that takes `stream`."""
    bad = []
    for mod, tree in _modules():
        for fn, calls in _functions(tree):
            if _is_helper(mod, fn) or "stream" not in _params(fn):
                continue
            bound = set()
            for node in ast.walk(fn):
                if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and _dotted(node.value.func) == "_lib.launch_stream":
                    bound |= {t.id for t in node.targets if isinstance(t, ast.Name)}
            for node in ast.walk(fn):
                if isinstance(node, ast.Attribute) and node.attr == "cuda_stream":
                    v = node.value
                    ok = (isinstance(v, ast.Name) and v.id in bound) or (isinstance(v, ast.Call) and _dotted(v.func) == "_lib.launch_stream")
                    if not ok:
                        bad.append("%s:%d %s" % (mod, node.lineno, fn.name))
    assert bad == [], "\n".join(bad)
