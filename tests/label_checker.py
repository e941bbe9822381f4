"""Segmentation checker -- TEST INFRASTRUCTURE ONLY (checker of aw_render_labels).

A thin layer over tests/rgb_checker.py: ``render_rgb`` already returns, per pixel, the render
entry of the nearest geom crossing (``geom``) and of the nearest visible-site crossing strictly in
front of it (``site``), found in fp64 on the oracle's poses.  The label rule of
include/adroit_wave.h (aw_render_labels) is the site where there is one and sites are drawn, else
the geom, else no entry.
"""
import numpy as np

AGREE = 0.995      # of a frame's pixels: the project's depth gate (test_cameras._check_frame's zok)


def entry_frame(ref, sites):
    """[H, W] render entries (-1: nothing) of a ``rgb_checker.render_rgb`` result"""
    lab = ref["geom"].astype(np.int64)
    if sites:
        lab = np.where(ref["site"] >= 0, ref["site"], lab)
    return lab


def apply_lut(entries, lut, background=-1):
    """the labels of an entry frame under a look-up table"""
    lut = np.asarray(lut)
    return np.where(entries >= 0, lut[np.maximum(entries, 0)], background)


def in_neighbourhood(got, want):
    """[H, W] bool: got[r, c] occurs among want[r-1:r+2, c-1:c+2] (the frame's edge replicated)"""
    H, W = want.shape
    pad = np.pad(want, 1, mode="edge")
    ok = np.zeros((H, W), bool)
    for dr in range(3):
        for dc in range(3):
            ok |= pad[dr:dr + H, dc:dc + W] == got
    return ok


def compare(got, want):
    """(fraction of pixels with the same label, number of differing pixels whose label is not in
    the 3x3 neighbourhood of the same pixel of ``want``)"""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    same = got == want
    stray = ~same & ~in_neighbourhood(got, want)
    return float(same.mean()), int(stray.sum())


def check_frame(got, want, what):
    """both conditions of the GPU tests; prints the figures before it asserts.  Agreement alone
    would pass a wrong label inside an object, the neighbourhood rule alone a frame shifted by a
    pixel: a label that differs must be a silhouette pixel, and there may be few of them."""
    agree, stray = compare(got, want)
    print(f"{what}: {agree:.5f} of pixels agree, {stray} differing pixels off a silhouette")
    assert agree >= AGREE, (what, agree)
    assert stray == 0, (what, stray)
