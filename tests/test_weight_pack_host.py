"""The fragment-ordered pack of a recurrent kernel (fov_lstm_pack_r, include/fov360.h) against the addresses the cluster
kernel's unpacked loader uses (lstm_cluster.hip: load_weights / load_r_block): for every workgroup slice, wave, lane and
register (j, s, g) the packed loader (load_r_block_packed) must fetch the element of R the unpacked one does - the registers
then hold the same values and the fused call's results cannot differ.  No GPU: both address computations are transcribed here."""
import numpy as np
import pytest

WIDTHS = (64, 128, 256)


def pack_r(R):
    """The pack as include/fov360.h defines it: element ((((c*NQ + jj)*4 + s)*64 + lane)*4 + g), lane = 16*g4 + n, is
    R[16*jj + 4*g4 + s][g*H + 16*c + n]."""
    H = R.shape[0]
    assert R.shape == (H, 4 * H)
    NQ = H // 16
    c, jj, s, g4, n, g = np.meshgrid(np.arange(NQ), np.arange(NQ), np.arange(4), np.arange(4), np.arange(16), np.arange(4), indexing="ij")
    return np.ascontiguousarray(R[16 * jj + 4 * g4 + s, g * H + 16 * c + n]).reshape(-1)


def loader_indices(H):
    """Flat element indices, one per (slice, wave, lane, j, s, g): where load_weights reads R, where load_r_block_packed reads
    the pack.  Byte offsets of the kernel divided by four."""
    G, NQ, H4 = H // 64, H // 16, 4 * H
    sl, wave, lane, j, s, g = np.meshgrid(np.arange(G), np.arange(4), np.arange(64), np.arange(NQ), np.arange(4), np.arange(4), indexing="ij")
    n, g4 = lane & 15, lane >> 4
    col0 = sl * 64 + wave * 16
    # load_weights: voff = (4*g4*H4 + col0 + n), kb = (((slice + (j>>2)) & (G-1))*64 + (j&3)*16)*H4, + s*H4 + g*H
    unpacked = (4 * g4 * H4 + col0 + n) + (((sl + (j >> 2)) & (G - 1)) * 64 + (j & 3) * 16) * H4 + s * H4 + g * H
    # load_r_block_packed: voff = (col0>>4)*NQ*4096 + lane*16 bytes, kb = (((slice + (j>>2)) & (G-1))*4 + (j&3))*4096, + s*1024;
    # register g is dword g of the 16-byte load
    packed = (col0 >> 4) * NQ * 1024 + lane * 4 + (((sl + (j >> 2)) & (G - 1)) * 4 + (j & 3)) * 1024 + s * 256 + g
    return unpacked.reshape(-1), packed.reshape(-1)


@pytest.mark.parametrize("H", WIDTHS)
def test_pack_is_a_permutation_of_r(H):
    R = np.arange(H * 4 * H, dtype=np.int64).reshape(H, 4 * H)      # every element its own flat index
    p = pack_r(R)
    assert p.shape == (H * 4 * H,)
    assert np.array_equal(np.sort(p), np.arange(H * 4 * H))


@pytest.mark.parametrize("H", WIDTHS)
def test_packed_loader_fetches_what_the_unpacked_loader_fetches(H):
    R = np.arange(H * 4 * H, dtype=np.int64).reshape(H, 4 * H)
    p = pack_r(R)
    unpacked, packed = loader_indices(H)
    assert unpacked.size == H * 4 * H                                   # the G x 4 waves' slices cover R ...
    assert unpacked.min() >= 0 and unpacked.max() < H * 4 * H and packed.min() >= 0 and packed.max() < H * 4 * H
    assert np.array_equal(np.sort(unpacked), np.arange(H * 4 * H))      # ... each element in exactly one register
    assert np.array_equal(p[packed], R.reshape(-1)[unpacked])


@pytest.mark.parametrize("H", WIDTHS)
def test_a_wave_instruction_reads_one_contiguous_kilobyte(H):
    """The point of the layout: the 64 lanes x 4 dwords of one packed load are 256 consecutive floats, 1 KB-aligned."""
    _, packed = loader_indices(H)
    G, NQ = H // 64, H // 16
    per_load = packed.reshape(G, 4, 64, NQ, 4, 4).transpose(0, 1, 3, 4, 2, 5).reshape(-1, 256)    # (slice, wave, j, s) x (lane, g)
    assert (per_load[:, 0] % 256 == 0).all()
    assert (per_load == per_load[:, :1] + np.arange(256)).all()
