"""Plain references for the streaming kernels of csrc/adam.hip and csrc/rows.hip, and a mirror of the geometry buffer's layout.

adam_step_ref : one Adam step in float64, in the operation order of adam.hip's head comment (torch's _single_tensor_adam).
geom_bytes / tiles_touched_offset / masked_geom : csrc/common.h geom_layout restated, and a geometry buffer that holds nothing
    but a header and a tiles_touched array -- what lr_adam_step_masked reads of it.
select_ref    : lr_select_rows as boolean indexing into a sentinel-filled destination.
pack_ply_ref  : lr_pack_ply_rows as the column order of save_ply.
"""
import torch

GEOM_FILL = 0xA5            # every byte of masked_geom that is neither header nor tiles_touched


def adam_step_ref(p, g, m, v, lr, b1, b2, eps, step):
    """New (p, m, v) as float64 tensors; nothing is modified in place."""
    p, g, m, v = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in (p, g, m, v))
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps
    p = p - (lr / (1.0 - b1 ** step)) * m / denom
    return p, m, v


def align256(n):
    return (n + 255) // 256 * 256


def tiles_touched_offset(P):
    """header, GaussRec[P] (48 bytes each), clamped[P] bytes: then tiles_touched (uint32 per Gaussian)."""
    return 256 + align256(48 * P) + align256(P)


def geom_bytes(P):
    """... followed by vis_list and offsets (uint32 each) and hitrec (16 bytes each)."""
    return tiles_touched_offset(P) + 3 * align256(4 * P) + align256(16 * P)


def masked_geom(P, touched_u32, overflow, device):
    """A geometry buffer of lr_geom_bytes(P) bytes of which only the header (zeros, word 1 = overflow) and tiles_touched are
    meaningful; every other byte is 0xA5, so that any other field read in place of the mask is garbage.  touched_u32: P values
    below 2^32 (any integer tensor)."""
    from luciddreamer_amd import _lib
    total = int(_lib.lib().lr_geom_bytes(P))
    assert total == geom_bytes(P), (P, total, geom_bytes(P))
    touched = torch.as_tensor(touched_u32).to("cpu", torch.int64).reshape(-1)
    assert touched.numel() == P and int(touched.min()) >= 0 and int(touched.max()) < 2 ** 32
    buf = torch.full((total,), GEOM_FILL, dtype=torch.uint8)
    buf[:256] = 0
    words = buf[:256].view(torch.int32)
    words[1] = int(overflow)
    off = tiles_touched_offset(P)
    as_i32 = torch.where(touched >= 2 ** 31, touched - 2 ** 32, touched).to(torch.int32)
    buf[off:off + 4 * P] = as_i32.view(torch.uint8)
    return buf.to(device)


def select_ref(src, mask, dst_sentinel, off):
    """Rows of src where mask != 0, in source order, written at row `off` of a copy of dst_sentinel; returns (dst, count)."""
    sel = src[mask != 0]
    dst = dst_sentinel.clone()
    dst[off:off + sel.shape[0]] = sel
    return dst, int(sel.shape[0])


def pack_ply_ref(xyz, f_dc, f_rest, opacity, scaling, rotation):
    """[P, 17 + 3 * n_rest]: x y z, three zero normals, f_dc, f_rest channel-major, opacity, scale, rot (save_ply's columns)."""
    P = xyz.shape[0]
    return torch.cat([xyz, torch.zeros_like(xyz), f_dc.transpose(1, 2).flatten(1), f_rest.transpose(1, 2).flatten(1),
                      opacity.reshape(P, 1), scaling, rotation], dim=1)
