"""cs16 input at the C ABI and in the binding, as far as it goes without a device: the sample-size export, which formats the create
calls let through to the device check, and the binding's refusal of a wrong host array on a cs16 object."""
import ctypes as C

import numpy as np
import pytest

import ddn


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except ImportError:
        return True


def test_input_format_bytes(built):
    l = ddn.lib()
    assert (ddn.IN_CU8, ddn.IN_CF32, ddn.IN_CS16) == (0, 1, 2)
    assert [l.ddn_input_format_bytes(f) for f in (ddn.IN_CU8, ddn.IN_CF32, ddn.IN_CS16)] == [2, 8, 4]
    assert l.ddn_input_format_bytes(-1) == 0 and l.ddn_input_format_bytes(3) == 0


def _create_batch(fmt):
    cfg = ddn.FrontEndConfig(2, 48000, 4800, 4, ddn.LPF_P25_C4FM, fmt, 4096, 0.0)
    h = C.c_void_p()
    rc = ddn.lib().ddn_batch_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        ddn.lib().ddn_batch_destroy(h)
    return rc, ddn.lib().ddn_last_error().decode()


def _create_cqpsk(fmt):
    cfg = ddn.CqpskConfig(2, 24000, 4800, ddn.LPF_P25_CQPSK, 1, fmt, 4096, 0.0)
    h = C.c_void_p()
    rc = ddn.lib().ddn_cqpsk_batch_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        ddn.lib().ddn_cqpsk_batch_destroy(h)
    return rc, ddn.lib().ddn_last_error().decode()


@pytest.mark.parametrize("create", [_create_batch, _create_cqpsk])
def test_create_accepts_cs16_up_to_the_device_check(built, create):
    """format 2 passes the argument checks: without a device the answer is DDN_ENODEV (it was DDN_EINVAL before cs16 existed), with
    one the object is made"""
    rc, _ = create(ddn.IN_CS16)
    assert rc == (ddn.DDN_ENODEV if _no_gpu() else ddn.DDN_OK)


@pytest.mark.parametrize("create,name", [(_create_batch, "ddn_batch_create"), (_create_cqpsk, "ddn_cqpsk_batch_create")])
def test_create_refuses_an_unknown_format_by_name(built, create, name):
    for fmt in (3, -1):
        rc, msg = create(fmt)
        assert rc == ddn.DDN_EINVAL and name in msg and "input_format" in msg, (rc, msg)


def _chain_creates():
    l = ddn.lib()

    def p25(fmt):
        cfg = ddn.P25ChainConfig(2, 16384, 8192, fmt, 1, 0, 0, 0, 0, 0, 0, 0.0, 0)
        h = C.c_void_p()
        return l.ddn_p25_chain_create(C.byref(cfg), C.byref(h))

    def node(fmt):
        cfg = ddn.NodeConfig(2, 16384, 8192, fmt, 1, 0, 0, 0, 0, 0, 0, None, None, None)
        h = C.c_void_p()
        return l.ddn_node_create(C.byref(cfg), C.byref(h))

    return [(p25, "ddn_p25_chain_create"), (node, "ddn_node_create")]


def test_chain_and_node_creates_refuse_an_unknown_format_by_name(built):
    for fn, name in _chain_creates():
        rc = fn(3)
        msg = ddn.lib().ddn_last_error().decode()
        assert rc == ddn.DDN_EINVAL and name in msg and "input_format" in msg, (name, rc, msg)


class _NoCalls:
    """stands where the library would be: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the binding called %s before refusing the array" % name)


@pytest.mark.parametrize("kind", ["batch", "cqpsk"])
def test_binding_refuses_wrong_arrays_on_a_cs16_object_before_any_c_call(built, kind, monkeypatch):
    B, n = 2, 100
    if kind == "batch":
        obj = ddn.Batch.__new__(ddn.Batch)
        obj.cfg = ddn.FrontEndConfig(B, 48000, 4800, 4, ddn.LPF_P25_C4FM, ddn.IN_CS16, 4096, 0.0)
        run = lambda a: obj.run_host(a, n)
    else:
        obj = ddn.CqpskBatch.__new__(ddn.CqpskBatch)
        obj.B = B
        obj.cfg = ddn.CqpskConfig(B, 24000, 4800, ddn.LPF_P25_CQPSK, 1, ddn.IN_CS16, 4096, 0.0)
        run = lambda a: obj.run(a)
    obj.h = C.c_void_p()
    monkeypatch.setattr(ddn, "lib", lambda: _NoCalls())
    with pytest.raises(TypeError):
        run(np.zeros((B, n, 2), np.float32))
    with pytest.raises(TypeError):
        run(np.zeros((B, n, 2), np.uint8))
    if kind == "batch":
        with pytest.raises(ValueError):
            run(np.zeros((B, n - 1, 2), np.int16))          # too few elements: the library would read past the array
    # the right array passes the check (and then reaches the library: the stand-in objects)
    with pytest.raises(AssertionError):
        run(np.zeros((B, n, 2), np.int16))
    # what the other formats accept is unchanged: no check of their own
    ddn.check_host_iq(ddn.IN_CU8, np.zeros(3, np.float32), B, n)
    ddn.check_host_iq(ddn.IN_CF32, np.zeros(3, np.uint8), B, n)
