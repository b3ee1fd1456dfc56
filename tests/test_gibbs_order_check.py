"""CPU: the checker of tests/test_gpu_gibbs_order.py tells numpy's summation order from a
sequential sum.  A numpy model of the Gibbs update (tests/gibbs_order.py model_rows) stands
in for the device: summing as numpy.sum it passes, with the very r it used; summing
sequentially it fails at every G >= 8, where the two orders part."""

import numpy
import pytest

import gibbs_order as go

G_LIST = [2, 3, 7, 8, 9, 63, 64, 65, 120, 121, 127, 128, 129, 136, 512, 513]


def _seq(a):
    return numpy.cumsum(a)[-1]


@pytest.mark.parametrize("G", G_LIST)
def test_checker_accepts_numpy_order_and_rejects_sequential(G):
    C, P, n = 65, 2, 2
    value, mu, s2 = go.start(C, P, G, G)
    _, _, hz, hu = go.variates(C, P, G, n, G)
    good = go.model_rows(value, s2, hz, hu, numpy.sum)
    share = go.check(good, s2, hz, hu, G, P, ("numpy", G))
    if G < 8:   # numpy's order is the sequential one
        assert share == 0.0
        go.check(go.model_rows(value, s2, hz, hu, _seq), s2, hz, hu, G, P, ("sequential", G))
        return
    assert share >= 0.20, share
    with pytest.raises(AssertionError):
        go.check(go.model_rows(value, s2, hz, hu, _seq), s2, hz, hu, G, P, ("sequential", G))
