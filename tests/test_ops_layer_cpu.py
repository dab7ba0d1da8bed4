"""The operator layer's host rules, without a GPU: how `ops.launch` marshals a wrapper's arguments (against a recording stub in place
of the library) and which forms `PackedConv.forms()` yields."""
import ctypes as C

import torch

from tdvc_amd import _lib as L
from tdvc_amd import ops

STREAM = 0x5A5A0


class _Recorder:
    """stands in for the loaded library: every entry point records (name, args); size queries answer 24, launches 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 24 if name.endswith("_work_floats") else 0
        return entry


ANY = object()          # an argument the wrapper makes itself (a workspace's address)


def _fm(c=8, dtype=torch.float16):
    return ops.FM(torch.zeros((1, 3, 5, c), dtype=dtype))


def _check_call(call, name, expect):
    got_name, args = call
    assert got_name == name
    argtypes = L.SIGNATURES[name][1]
    assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} declared"
    for i, (a, t) in enumerate(zip(args, argtypes)):
        t.from_param(a)                                            # raises where ctypes would refuse the argument
    assert len(expect) == len(args) - 1
    for i, (a, e) in enumerate(zip(args, expect)):
        if isinstance(e, ops.FM):
            assert isinstance(a, L.FMapDesc) and bytes(a) == bytes(e.desc()), f"{name}: argument {i} is not the map's descriptor"
        elif isinstance(e, torch.Tensor):
            assert type(a) is int and a == e.data_ptr(), f"{name}: argument {i} is not the tensor's address"
        elif e is None:
            assert a is None, f"{name}: argument {i} should be absent"
        elif e is ANY:
            assert type(a) is int and a != 0
        else:
            assert a == e and type(a) is type(e), f"{name}: argument {i}"
    last = args[-1]
    assert (last.value if isinstance(last, C.c_void_p) else last) == STREAM, f"{name}: the last argument is not the forced stream"


def test_launch_rule_marshals_every_kind_of_argument(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    monkeypatch.setattr(ops, "FORCE_STREAM", STREAM)
    monkeypatch.setattr(ops, "TAPE", None)
    a, b, c, d = _fm(), _fm(), _fm(), _fm()
    v, gate, dgate = torch.zeros(8), torch.zeros((1, 8)), torch.zeros((1, 8))

    cases = []                                                     # (entry point, the arguments it must have received, stream apart)
    ops.copy_cast(a, b)
    cases.append(("tdvc_copy_cast", [a, b]))
    assert ops.act_backward(a, b, ops.ACT_LRELU, 0.1, res=None) is a
    cases.append(("tdvc_act_backward", [a, b, None, ops.ACT_LRELU, 0.1, a]))
    ops.act_backward(a, b, ops.ACT_RELU, 0.0, res=c, out=d)
    cases.append(("tdvc_act_backward", [a, b, c, ops.ACT_RELU, 0.0, d]))
    ops.bcast_channel_add(a, v, 0.5)
    cases.append(("tdvc_bcast_channel_add", [a, v, 0.5]))
    ops.gate_backward(a, b, gate, None, dgate)
    cases.append(("tdvc_gate_backward_work_floats", None))        # the size query keeps its own call: no stream, no check
    cases.append(("tdvc_gate_backward", [a, b, gate, None, dgate, ANY, 24]))
    ops.quantize(a, b)
    cases.append(("tdvc_quantize", [a, None, b]))
    ops.quantize(a, b, noise=c)
    cases.append(("tdvc_quantize", [a, c, b]))
    for g_ in (None, gate):
        for r_ in (None, c):
            for o2 in (None, d):
                ops.scale_act_res(a, b, gate=g_, act=ops.ACT_RELU, slope=0.0, res=r_, res_sign=-1.0, out2=o2)
                cases.append(("tdvc_scale_act_res", [a, g_, ops.ACT_RELU, 0.0, r_, -1.0, b, o2]))

    assert len(rec.calls) == len(cases)
    for call, (name, expect) in zip(rec.calls, cases):
        if expect is None:
            assert call == (name, (a.N, a.C))
        else:
            _check_call(call, name, expect)


def test_launch_names_the_call_in_its_error(monkeypatch):
    class Failing(_Recorder):
        def __getattr__(self, name):
            if name == "tdvc_last_error":
                return lambda: b"boom"
            return lambda *args: -3
    fail = Failing()
    monkeypatch.setattr(L, "lib", lambda: fail)
    monkeypatch.setattr(ops, "FORCE_STREAM", STREAM)
    for call, text in ((lambda: ops.copy_cast(_fm(), _fm()), "copy_cast: rc=-3: boom"),
                       (lambda: ops.launch("tdvc_copy_cast", _fm(), _fm(), what="cast"), "cast: rc=-3: boom")):
        try:
            call()
        except L.TdvcHipError as e:
            assert str(e) == text
        else:
            raise AssertionError("a non-zero return code did not raise")
    assert ops.launch("tdvc_copy_cast", _fm(), _fm(), check=False) == -3


def _pc():
    return ops.PackedConv(torch.zeros(16, dtype=torch.uint8), torch.zeros(32), 8, 8, 1, 1, 1, 0, 8, [(0, 0)])


def test_forms_yields_every_derived_form_once():
    before = ops.FORMS_CREATED
    layer, other, dgrad, plain, column = _pc(), _pc(), _pc(), _pc(), _pc()
    assert ops.FORMS_CREATED == before + 5
    assert list(layer.forms()) == [] and layer.plain is None and layer.column is None and layer.dgrad is None
    layer.dgrad = dgrad
    dgrad.plain, dgrad.column = plain, column          # the dgrad form has forms of its own
    layer.column = other.column = column               # and the column form has two more parents
    got = list(layer.forms())
    assert sorted(map(id, got)) == sorted(map(id, (dgrad, plain, column))) and got[0] is dgrad
    seen = set()                                       # a walk over several layers (PackBatch): what one layer yielded, the next does not
    walk = list(layer.forms(seen)) + list(other.forms(seen))
    assert sorted(map(id, walk)) == sorted(map(id, (dgrad, plain, column)))
    assert [id(f) for f in other.forms()] == [id(column)]


def test_keyed_cache_rebuilds_under_another_key():
    k, built = ops._Keyed(), []
    make = lambda v: (lambda: built.append(v) or v)
    assert k.of("tables", 64, make("a")) == "a" and k.of("tables", 64, make("b")) == "a"
    assert k.of("tables", 72, make("c")) == "c" and k.of("work", 64, make("d")) == "d"          # another channel count; another slot
    assert built == ["a", "c", "d"]
    assert _pc().wgrad is not _pc().wgrad and _pc().tmpl == {}
