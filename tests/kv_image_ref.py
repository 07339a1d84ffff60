"""A plain-Python restatement of the KV image's layout (include/nano_mi355x.h "KV images"; the library's arithmetic is
nano_amd/csrc/kv_image.h).  64-byte little-endian header, then the payload block-major: block b = positions 64 b .. min(64 b + 63,
n_pos - 1), inside a block the layers ascending, per layer the block's K rows (one contiguous run) and then its V rows."""
import struct

import numpy as np

MAGIC, VERSION, HEADER_BYTES, BLOCK_ROWS = b"NKV1", 1, 64, 64
FMT_BYTES = {0: 4, 1: 2, 2: 1}                    # element format -> bytes: FP32, FP16, FP8 e4m3
HEADER = struct.Struct("<4s9IQQ2I")               # magic, version, header bytes, format, n_layer, kv_dim, n_pos, block rows, row bytes, 0, payload, tag, 0, 0
assert HEADER.size == HEADER_BYTES


def blocks(n_pos):
    return (n_pos + BLOCK_ROWS - 1) // BLOCK_ROWS


def block_rows(n_pos, block):
    """rows per run of `block` in the image of n_pos positions"""
    return min(BLOCK_ROWS, n_pos - BLOCK_ROWS * block)


def vec_bytes(row_bytes):
    return 16 if row_bytes % 16 == 0 else 8 if row_bytes % 8 == 0 else 4


def plan(n_layer, kv_dim, elem_bytes, n_pos):
    rb = kv_dim * elem_bytes
    payload = n_pos * n_layer * 2 * rb
    return {"header_bytes": HEADER_BYTES, "payload_bytes": payload, "total_bytes": HEADER_BYTES + payload, "blocks": blocks(n_pos),
            "last_rows": block_rows(n_pos, blocks(n_pos) - 1) if n_pos else 0, "block_stride": BLOCK_ROWS * n_layer * 2 * rb,
            "vec_bytes": vec_bytes(rb), "_zero": 0}


def offset(n_layer, row_bytes, n_pos, block, layer, kv, row):
    """byte offset, from the start of the image of n_pos positions, of row `row` (position 64 block + row) of layer `layer`'s K (kv = 0)
    or V (kv = 1) run"""
    assert 0 <= row < block_rows(n_pos, block) and 0 <= layer < n_layer and kv in (0, 1)
    return HEADER_BYTES + BLOCK_ROWS * block * n_layer * 2 * row_bytes + ((layer * 2 + kv) * block_rows(n_pos, block) + row) * row_bytes


def model_tag(desc_words, params_bytes):
    """FNV-1a (64 bit) over the twelve NanoModelDesc words and params_bytes, little-endian bytes: a guard against mixed-up shapes"""
    h = 0xCBF29CE484222325
    for b in struct.pack("<12IQ", *[int(w) for w in desc_words], int(params_bytes)):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def header(fmt, n_layer, kv_dim, n_pos, tag=0):
    rb = kv_dim * FMT_BYTES[fmt]
    return HEADER.pack(MAGIC, VERSION, HEADER_BYTES, fmt, n_layer, kv_dim, n_pos, BLOCK_ROWS, rb, 0, n_pos * n_layer * 2 * rb, tag, 0, 0)


def write(k, v, fmt, tag=0):
    """the image of rows k, v: uint8 arrays [n_layer][n_pos][row_bytes] (the cache's own bytes)"""
    k, v = np.asarray(k, np.uint8), np.asarray(v, np.uint8)
    n_layer, n_pos, rb = k.shape
    assert v.shape == k.shape and rb % FMT_BYTES[fmt] == 0
    img = np.zeros(HEADER_BYTES + n_pos * n_layer * 2 * rb, np.uint8)
    img[:HEADER_BYTES] = np.frombuffer(header(fmt, n_layer, rb // FMT_BYTES[fmt], n_pos, tag), np.uint8)
    for b in range(blocks(n_pos)):
        r = block_rows(n_pos, b)
        for layer in range(n_layer):
            for kv, src in enumerate((k, v)):
                o = offset(n_layer, rb, n_pos, b, layer, kv, 0)
                img[o:o + r * rb] = src[layer, 64 * b:64 * b + r].reshape(-1)
    return img


def read(img):
    """(header fields as a dict, k, v) of an image: the inverse of write()"""
    img = np.asarray(img, np.uint8)
    f = HEADER.unpack(img[:HEADER_BYTES].tobytes())
    h = dict(zip(("magic", "version", "header_bytes", "format", "n_layer", "kv_dim", "n_pos", "block_rows", "row_bytes", "reserved0",
                  "payload_bytes", "model_tag", "reserved1a", "reserved1b"), f))
    n_layer, n_pos, rb = h["n_layer"], h["n_pos"], h["row_bytes"]
    k, v = np.zeros((n_layer, n_pos, rb), np.uint8), np.zeros((n_layer, n_pos, rb), np.uint8)
    for b in range(blocks(n_pos)):
        r = block_rows(n_pos, b)
        for layer in range(n_layer):
            for kv, dst in enumerate((k, v)):
                o = offset(n_layer, rb, n_pos, b, layer, kv, 0)
                dst[layer, 64 * b:64 * b + r] = img[o:o + r * rb].reshape(r, rb)
    return h, k, v


def prefix(img, n):
    """the image of the first n positions, cut out of the image of more: the header with n_pos and the payload size replaced, the
    byte prefix of the whole blocks, and the row cut inside the block that n ends in"""
    img = np.asarray(img, np.uint8)
    f = list(HEADER.unpack(img[:HEADER_BYTES].tobytes()))
    n_layer, n_pos, rb = f[4], f[6], f[8]
    assert n <= n_pos
    f[6], f[10] = n, n * n_layer * 2 * rb
    full, part = divmod(n, BLOCK_ROWS)
    stride = BLOCK_ROWS * n_layer * 2 * rb
    out = [np.frombuffer(HEADER.pack(*f), np.uint8), img[HEADER_BYTES:HEADER_BYTES + full * stride]]
    if part:
        for layer in range(n_layer):
            for kv in (0, 1):
                o = offset(n_layer, rb, n_pos, full, layer, kv, 0)
                out.append(img[o:o + part * rb])
    return np.concatenate(out)
