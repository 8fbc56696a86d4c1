"""Winograd position 5 of a row's last tile is dead where W % 4 != 0 (csrc/winograd.hip, the skip5 form of kstep): in F(4,3) only the
fourth output of a tile reads m5 (y3 = (m1 - m2) + 8 (m3 - m4) + m5), and that pixel of the last tile lies at wo >= W.  Stated on
the CPU with the fp32 Winograd statement of tests/encoder_sweep_ref.py: with position 5 of every row's last tile put to zero (what
the accumulator of a wave that skips it holds) every output with wo < W stays bit-for-bit what it was, for W = 5, 6, 7 (Tw = 2) and
W = 11 (Tw = 3).  Controls: the same zeroing changes the dropped pixel, and changes a stored one where W % 4 == 0."""
import pytest
import torch

import encoder_sweep_ref as R


def products(x, w_ohwi):
    """m [6][n][h][tw][cout] of R.wino43_conv in float32: the same input transform, the same einsum per kernel row, the same order"""
    n, h, wd, c = x.shape
    co, tw = w_ohwi.shape[0], (wd + 3) // 4
    u = R.wino43_weights(w_ohwi, torch.float32)
    xp = torch.zeros((n, h + 2, 4 * tw + 2, c), dtype=torch.float32)
    xp[:, 1:h + 1, 1:wd + 1] = x
    d = xp.unfold(2, 6, 4)
    d0, d1, d2, d3, d4, d5 = (d[..., i] for i in range(6))
    s12, q12 = -4.0 * d2 + d4, 4.0 * d1 - d3
    s34, q34 = d4 - d2, 2.0 * d3 - 2.0 * d1
    v = torch.stack([(4.0 * d0 - 5.0 * d2) + d4, s12 - q12, s12 + q12, s34 + q34, s34 - q34, (4.0 * d1 - 5.0 * d3) + d5])
    m = torch.zeros((6, n, h, tw, co), dtype=torch.float32)
    for kh in range(3):
        m = m + torch.einsum("xnhtc,xoc->xnhto", v[:, :, kh:kh + h], u[:, :, kh, :])
    return m


def outputs(m):
    """y [n][h][4 tw][cout] = A^T m in the epilogue's association, the padded columns kept"""
    m0, m1, m2, m3, m4, m5 = m
    a12, b12, a34, b34 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    t = b34 + b34
    y = torch.stack([(m0 + a12) + a34, b12 + t, a12 + 4.0 * a34, (b12 + 4.0 * t) + m5], dim=3)
    n, h, tw, _, co = y.shape
    return y.reshape(n, h, 4 * tw, co)


def operands(wd, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((3, 4, wd, 20), generator=g)
    w = torch.randn((12, 3, 3, 20), generator=g) * (2.0 / 180) ** 0.5
    return x, w


@pytest.mark.parametrize("wd", [5, 6, 7, 11])
def test_dead_position_leaves_every_stored_pixel_bitwise(wd):
    x, w = operands(wd, 40 + wd)
    m = products(x, w)
    y = outputs(m)
    assert torch.equal(y[:, :, :wd], R.wino43_conv(x, w, torch.float32)), "this file's statement is not the reference statement"
    dead = m.clone()
    dead[5, :, :, -1, :] = 0.0
    yd = outputs(dead)
    assert torch.equal(yd[:, :, :wd], y[:, :, :wd])
    # control: the zeroing is seen by the pixel that reads position 5, which is outside the image
    assert not torch.equal(yd[:, :, -1], y[:, :, -1])
    assert torch.equal(yd[:, :, :-1], y[:, :, :-1])


def test_whole_last_tile_needs_position_five():
    """W % 4 == 0: the last tile's fourth pixel is stored, so the kernel must keep all six positions there"""
    x, w = operands(8, 48)
    m = products(x, w)
    y = outputs(m)
    assert torch.equal(y, R.wino43_conv(x, w, torch.float32))
    dead = m.clone()
    dead[5, :, :, -1, :] = 0.0
    assert not torch.equal(outputs(dead)[:, :, 7], y[:, :, 7])
