"""helpers.options, the one way the tests change options on a shared device: what it promises, on a host-only context (no GPU)."""
import pytest

import fraytracer_amd as ft
from helpers import option_defaults, options


@pytest.fixture
def dev():
    d = ft.Device(-1)
    yield d
    d.close()


def snapshot(dev):
    return {k: dev.get_option(k) for k in ft.Device.OPTIONS}


def test_defaults_are_the_librarys(dev):
    assert option_defaults() == snapshot(dev) and set(option_defaults()) == set(ft.Device.OPTIONS)


def test_restores_the_values_found_not_the_defaults(dev):
    dev.set_option("tail_k", 3)
    with options(dev, tail_k=64, cull=0):
        assert (dev.get_option("tail_k"), dev.get_option("cull")) == (64, 0)
    assert dev.get_option("tail_k") == 3 and dev.get_option("cull") == 1


def test_restores_when_the_body_raises(dev):
    dev.set_option("tail_k", 3)
    before = snapshot(dev)
    with pytest.raises(ZeroDivisionError):
        with options(dev, tail_k=64, cull=0):
            1 / 0
    assert snapshot(dev) == before


def test_restores_what_the_setter_changed(dev):
    dev.set_option("reuse", 0)
    before = snapshot(dev)
    with options(dev, cert=0) as set_:
        set_(reuse=1, chunk=32)
        set_(reuse=0, chunk=16, cert=1)                  # a second change keeps the first-seen old value
        assert (dev.get_option("reuse"), dev.get_option("chunk"), dev.get_option("cert")) == (0, 16, 1)
    assert snapshot(dev) == before


def test_an_unknown_name_raises_and_changes_nothing(dev):
    before = snapshot(dev)
    with pytest.raises(KeyError):
        with options(dev, cull=0, no_such_option=1):
            pytest.fail("the body must not run")
    assert snapshot(dev) == before
    with options(dev, cull=0) as set_:
        with pytest.raises(KeyError):
            set_(tail_k=8, no_such_option=1)
        assert dev.get_option("tail_k") == -1 and dev.get_option("cull") == 0
    assert snapshot(dev) == before


def test_a_refused_value_raises_and_the_options_before_it_are_back(dev):
    dev.set_option("tail_k", 3)
    before = snapshot(dev)
    with pytest.raises(ft.FrayTracerError):
        with options(dev, tail_k=64, cull=0, order=3, reuse=0):
            pytest.fail("the body must not run")
    assert snapshot(dev) == before


def test_nested_scopes_unwind_in_order(dev):
    with options(dev, tail_k=8, cull=0):
        with options(dev, tail_k=16) as set_:
            set_(cull=1, guided=1)
            with options(dev, tail_k=32, guided=0):
                assert (dev.get_option("tail_k"), dev.get_option("cull"), dev.get_option("guided")) == (32, 1, 0)
            assert (dev.get_option("tail_k"), dev.get_option("cull"), dev.get_option("guided")) == (16, 1, 1)
        assert (dev.get_option("tail_k"), dev.get_option("cull"), dev.get_option("guided")) == (8, 0, 0)
    assert snapshot(dev) == option_defaults()
