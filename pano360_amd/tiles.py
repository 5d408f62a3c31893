"""Tile pyramids of a finished mosaic, for viewers that cannot open it as one file: a Deep Zoom
image of the flat mosaic (what OpenSeadragon and map-style viewers read) and a multiresolution cube
of the sphere (the layout Pannellum reads).

The names and rectangles are pure host functions (``tile_grid``, ``deepzoom_files``,
``multires_files``).  The pixels are on the device already: a Deep Zoom level is a level of
``view.mip_device``'s chain (both halve with the sizes rounded up), a cube level is
``view.render_device`` of ``view.cube_faces``.  Every tile is a crop view of one of those, never a
copy, and all tiles of a pyramid go to ``jpeg.encode_batch_device`` together: one native call as
far as its scratch budget allows, each file the bytes Pillow would write for that crop.  Both
layouts are written from the formats' descriptions and checked structurally (tests/test_tiles_host.py),
not in a viewer.
"""
import json
import os

from . import view as _view

DZI_NS = "http://schemas.microsoft.com/deepzoom/2008"
FACE_LETTERS = tuple(name[0] for name in _view.CUBE_FACES)          # f r b l u d


def tile_grid(h, w, tile):
    """The tiles of an h x w image, row by row: [(row, col, y0, x0, th, tw)].  Edge tiles are
    smaller, never padded."""
    h, w, tile = int(h), int(w), int(tile)
    if h < 1 or w < 1 or tile < 1:
        raise ValueError(f"a {h} x {w} image at tile {tile}: all >= 1")
    return [(row, col, y0, x0, min(tile, h - y0), min(tile, w - x0))
            for row, y0 in enumerate(range(0, h, tile))
            for col, x0 in enumerate(range(0, w, tile))]


# ------------------------------------------------------------------ Deep Zoom
def deepzoom_levels(h, w):
    """[(H_k, W_k)] of Deep Zoom levels k = 0 .. ceil(log2(max(h, w))): level 0 is 1 x 1, the top
    level the image; level k is level ``n - 1 - k`` of ``view.mip_shapes``.  Raises ValueError for
    an image the mip chain does not take down to 1 x 1."""
    shapes = _view.mip_shapes(h, w)
    if min(int(h), int(w)) < 1 or max(int(h), int(w)) > _view.MAX_SIDE or shapes[-1] != (1, 1):
        raise ValueError(f"a mosaic of {h} x {w}: sides 1 .. {_view.MAX_SIDE}")
    return shapes[::-1]


def deepzoom_files(h, w, tile):
    """The tiles of the Deep Zoom pyramid of an h x w image, overlap 0:
    [(name, mip level, y0, x0, th, tw)] with name = ``<k>/<col>_<row>.jpg`` under
    ``<stem>_files/``, levels ascending."""
    levels = deepzoom_levels(h, w)
    return [(f"{k}/{col}_{row}.jpg", len(levels) - 1 - k, y0, x0, th, tw)
            for k, (lh, lw) in enumerate(levels)
            for row, col, y0, x0, th, tw in tile_grid(lh, lw, tile)]


def dzi_xml(h, w, tile):
    """The Deep Zoom descriptor of an h x w image."""
    return ('<?xml version="1.0" encoding="UTF-8"?>\n'
            f'<Image xmlns="{DZI_NS}" Format="jpg" Overlap="0" TileSize="{int(tile)}">\n'
            f'  <Size Height="{int(h)}" Width="{int(w)}"/>\n'
            '</Image>\n')


def _mips(mosaic_or_mips, eng):
    if isinstance(mosaic_or_mips, _view.Mips):
        return mosaic_or_mips
    return _view.mip_device(mosaic_or_mips, eng)


def _write_files(paths, blobs):
    made = set()
    for path, blob in zip(paths, blobs):
        folder = os.path.dirname(path)
        if folder and folder not in made:
            os.makedirs(folder, exist_ok=True)
            made.add(folder)
        with open(path, "wb") as fid:
            fid.write(blob)


def deepzoom_tiles(mips, tile):
    """(names, crop views) of ``deepzoom_files`` on a mip chain: device tensors, no copies."""
    rows = deepzoom_files(mips.shape[0], mips.shape[1], tile)
    levels = {}
    views = []
    for _, l, y0, x0, th, tw in rows:
        if l not in levels:
            levels[l] = mips.level(l)
        views.append(levels[l][y0:y0 + th, x0:x0 + tw])
    return [r[0] for r in rows], views


def write_deepzoom(stem, mosaic_or_mips, tile=512, quality=75, eng=None, order="bgr"):
    """Writes ``<stem>.dzi`` and the tiles ``<stem>_files/<k>/<col>_<row>.jpg`` of a uint8
    [H][W][3] mosaic (device tensor, host array or its ``view.Mips``; ``order`` its channel
    order).  Returns the files written, the descriptor first.  A mosaic beyond the mip chain's
    limits raises ValueError."""
    from . import jpeg as _jpeg
    shape = mosaic_or_mips.shape[:2]
    deepzoom_levels(*shape)                             # (before anything is queued)
    tile_grid(1, 1, tile)
    mips = _mips(mosaic_or_mips, eng)
    names, views = deepzoom_tiles(mips, tile)
    blobs = _jpeg.encode_batch_device(views, quality, order=order, eng=eng)
    paths = [f"{stem}.dzi"] + [os.path.join(f"{stem}_files", *n.split("/")) for n in names]
    _write_files(paths, [dzi_xml(shape[0], shape[1], tile).encode()] + blobs)
    return paths


# -------------------------------------------------------------- cube multires
def multires_levels(side, tile):
    """(cube side, L): the largest ``tile * 2^(L - 1)`` not above ``side``; level l = 1 .. L has
    faces of side ``tile * 2^(l - 1)``, so every level is whole tiles."""
    side, tile = int(side), int(tile)
    if tile < 1 or side < tile:
        raise ValueError(f"a cube of side {side} at tile {tile}: side >= tile >= 1")
    levels = 1
    while tile << levels <= side:
        levels += 1
    return tile << (levels - 1), levels


def multires_files(side, tile):
    """The files of the cube pyramid: [(name, level, face, y0, x0, th, tw)], face an index into
    ``view.CUBE_FACES``; name = ``<l>/<s><row>_<col>.jpg`` with s the face's first letter, levels
    ascending, then ``fallback/<s>.jpg``, the level-1 faces."""
    _, levels = multires_levels(side, tile)
    rows = [(f"{l}/{s}{row}_{col}.jpg", l, face, y0, x0, th, tw)
            for l in range(1, levels + 1)
            for face, s in enumerate(FACE_LETTERS)
            for row, col, y0, x0, th, tw in tile_grid(tile << (l - 1), tile << (l - 1), tile)]
    return rows + [(f"fallback/{s}.jpg", 1, face, 0, 0, tile, tile)
                   for face, s in enumerate(FACE_LETTERS)]


def multires_config(side, tile):
    """``config.json`` of the cube pyramid."""
    cube, levels = multires_levels(side, tile)
    return {"type": "multires",
            "multiRes": {"path": "/%l/%s%y_%x", "fallbackPath": "/fallback/%s",
                         "extension": "jpg", "tileResolution": int(tile), "maxLevel": levels,
                         "cubeResolution": cube}}


def multires_tiles(mips, geom, side, tile, eng=None, background=None):
    """(names, crop views) of ``multires_files``: the faces of a level are one
    ``view.render_device`` launch from the mip chain; device tensors, no copies.  ``background`` =
    (``view.Mips`` or image, geometry) of ``fill.sphere_device``: the faces are rendered through
    ``fill.render_filled_device``, which takes what the mosaic does not cover from that sphere."""
    rows = multires_files(side, tile)
    if background is None:
        def render(views):
            return _view.render_device(mips, geom, views, eng)[0]
    else:
        from . import fill as _fill
        background = (_mips(background[0], eng), background[1])

        def render(views):
            return _fill.render_filled_device(mips, geom, views, background, eng)[0]
    faces = {l: render(_view.cube_faces(int(tile) << (l - 1)))
             for l in range(1, multires_levels(side, tile)[1] + 1)}
    return [r[0] for r in rows], [faces[l][face][y0:y0 + th, x0:x0 + tw]
                                  for _, l, face, y0, x0, th, tw in rows]


def write_multires(directory, mosaic_or_mips, geom, side, tile=512, quality=75, eng=None,
                   order="bgr", background=None):
    """Writes the cube pyramid of a mosaic with geometry ``geom`` (``view.MosaicGeometry``) into
    ``directory``: ``config.json``, ``<l>/<s><row>_<col>.jpg`` and ``fallback/<s>.jpg``.  All
    levels' tiles are coded together; tiles the mosaic does not cover are written too, black, or
    from ``background`` (see ``multires_tiles``) when it is given.
    Returns the files written, the configuration first."""
    from . import jpeg as _jpeg
    config = multires_config(side, tile)                # (before anything is queued)
    names, views = multires_tiles(_mips(mosaic_or_mips, eng), geom, side, tile, eng, background)
    blobs = _jpeg.encode_batch_device(views, quality, order=order, eng=eng)
    paths = [os.path.join(directory, "config.json")] + \
        [os.path.join(directory, *n.split("/")) for n in names]
    _write_files(paths, [(json.dumps(config, indent=2) + "\n").encode()] + blobs)
    return paths
