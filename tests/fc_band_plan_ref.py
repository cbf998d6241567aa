"""The band plan of k_fast_cells restated in Python (csrc/orb_host.cpp: level sizes, FAST cells, bands), for the tests of the
rejection test's item enumeration: which LDS tiles -- (pitch, bh, dw_lo, dw_hi) -- a frame size produces, and how many runs of 64
items each holds.  Host arithmetic only."""
import math

import numpy as np

EDGE, BORDER, PCAP, BAND_CELLS = 19, 16, 144, 4


def level_sizes(w, h, nlevels, scale_factor=1.2):
    f32 = np.float32
    scale, out = f32(1.0), []
    for l in range(nlevels):
        if l:
            scale = f32(scale * f32(scale_factor))
        inv = f32(1.0) / scale
        out.append((int(np.rint(f32(w) * inv)), int(np.rint(f32(h) * inv))))
    return out


def cells(lw, lh):
    """(x0, y0, cw, ch) of the level's FAST cells, row-major."""
    f32 = np.float32
    max_bx, max_by = lw - EDGE + 3, lh - EDGE + 3
    width, height = f32(max_bx - BORDER), f32(max_by - BORDER)
    ncols, nrows = int(width / f32(30)), int(height / f32(30))
    out = []
    if ncols < 1 or nrows < 1:
        return out
    wcell, hcell = int(math.ceil(width / f32(ncols))), int(math.ceil(height / f32(nrows)))
    for i in range(nrows):
        ini_y = BORDER + i * hcell
        if ini_y >= max_by - 3:
            continue
        max_y = min(ini_y + hcell + 6, max_by)
        for j in range(ncols):
            ini_x = BORDER + j * wcell
            if ini_x >= max_bx - 6:
                continue
            max_x = min(ini_x + wcell + 6, max_bx)
            out.append((ini_x, ini_y, max_x - ini_x, max_y - ini_y))
    return out


def bands(w, h, nlevels, scale_factor=1.2):
    """One dict per band of a w x h frame, levels in order: level, ncells, xa, y0, pitch, bh, c_lo, c_hi, dw_lo, dw_hi, cells
    (the band's (x0, y0, cw, ch))."""
    out = []
    for level, (lw, lh) in enumerate(level_sizes(w, h, nlevels, scale_factor)):
        cs = cells(lw, lh)
        a = 0
        while a < len(cs):
            x0, y0, cw, ch = cs[a]
            xa = (x0 - 4) & ~3
            b, pitch = a, 0
            while b < len(cs) and cs[b][1] == y0:
                p2 = (cs[b][0] + cs[b][2] + 4 - xa + 15) & ~15
                if b > a and (p2 > PCAP or b - a >= BAND_CELLS):
                    break
                pitch, b = p2, b + 1
            xl, _, cwl, _ = cs[b - 1]
            c_lo, c_hi = x0 + 3 - xa, xl + cwl - 3 - xa
            out.append(dict(level=level, ncells=b - a, xa=xa, y0=y0, pitch=pitch, bh=ch, c_lo=c_lo, c_hi=c_hi,
                            dw_lo=max(1, c_lo >> 2), dw_hi=min(pitch // 4 - 2, (c_hi - 1) >> 2), cells=cs[a:b]))
            a = b
    return out


def geometries(w, h, nlevels):
    """The distinct (pitch, bh, dw_lo, dw_hi) of the frame size's bands."""
    return sorted({(b["pitch"], b["bh"], b["dw_lo"], b["dw_hi"]) for b in bands(w, h, nlevels)})


def runs(g):
    pitch, bh, dw_lo, dw_hi = g
    return -(-max(bh - 6, 0) * max(dw_hi - dw_lo + 1, 0) // 64)


def wave_runs(g, waves=4):
    r = runs(g)
    return [(r - w + waves - 1) // waves for w in range(waves)]
