"""cf_average_create_budget holds a mean against the wet mask by the mask's own extent (include/coflux.h): a uint8 mask is
(nx + 2hx)(ny + 2hy) BYTES, so a mean that starts right behind it is legal, and a mean that shares one byte with it — from
either side — is refused; a bottom-height mask is as many doubles, and a mean one element inside it is refused.  The arrays are
carved out of one buffer, so their places do not depend on the allocator."""
import numpy as np
import pytest
import torch

from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import CofluxError, FluxContext

pytestmark = pytest.mark.gpu

NX, NY, HX, HY = 12, 4, 2, 2
N = (NX + 2 * HX) * (NY + 2 * HY)      # 128 cells: a uint8 mask of 128 bytes, a parent array of 1024


def _context(mask_kind):
    ctx = FluxContext(NX, NY, HX, HY, ic.flux_params(mask_kind=mask_kind), ring=0)
    heat = ctx.to_device(np.full(ctx.shape, 2.5))
    return ctx, heat


def _make(ctx, heat, mask, mean):
    return ctx.budget_average([("heat_ice_ocean", 1.0, mean)], ocean=dict(mask=mask), ice=dict(interface_heat=heat))


def _doubles(raw, first_byte):
    """A mean of the context's shape whose first byte is byte `first_byte` of the uint8 buffer `raw` (a multiple of 8)."""
    return raw[first_byte:first_byte + 8 * N].view(torch.float64).view(NY + 2 * HY, NX + 2 * HX)


def test_a_mean_right_behind_a_uint8_mask_is_accepted_and_one_that_shares_a_byte_is_refused():
    ctx, heat = _context(abi.MASK_U8)
    try:
        raw = torch.zeros(8 * N + N + 8 * N + 64, dtype=torch.uint8, device="cuda")
        mask = raw[8 * N:8 * N + N].view(NY + 2 * HY, NX + 2 * HX)
        mask.fill_(1)
        # right behind the mask's last byte, and ending right at its first: no byte shared
        for first in (8 * N + N, 0):
            mean = _doubles(raw, first)
            mean.fill_(float("nan"))
            avg = _make(ctx, heat, mask, mean)
            avg.collect(1.0)
            ctx.sync()
            inner = mean[HY:HY + NY, HX:HX + NX]
            assert torch.isfinite(inner).all() and (inner != 0).all(), first
            assert (mask == 1).all(), "the collection wrote into the mask"
            avg.close()
        # one byte shared: the mean's first element is the mask's last eight bytes; its last element the mask's first eight
        for first in (8 * N + N - 8, 8):
            with pytest.raises(CofluxError, match="overlaps the mask"):
                _make(ctx, heat, mask, _doubles(raw, first))
    finally:
        ctx.close()


def test_a_bottom_height_mask_keeps_a_whole_parent_array():
    ctx, heat = _context(abi.MASK_BOTTOM_HEIGHT)
    try:
        buf = torch.zeros(3 * N, dtype=torch.float64, device="cuda")
        shape = (NY + 2 * HY, NX + 2 * HX)
        mask = buf[N:2 * N].view(shape)
        mask.fill_(-100.0)
        for first in (2 * N, 0):
            _make(ctx, heat, mask, buf[first:first + N].view(shape)).close()
        for first in (2 * N - 1, 1):
            with pytest.raises(CofluxError, match="overlaps the mask"):
                _make(ctx, heat, mask, buf[first:first + N].view(shape))
    finally:
        ctx.close()
