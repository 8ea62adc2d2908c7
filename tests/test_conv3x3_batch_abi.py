"""toda_conv3x3_transform_weight_batch validates its table on the host before anything is launched: no GPU needed."""
import ctypes

from toda_amd import lib as L


def test_batch_transform_validates_every_entry_before_it_launches():
    lib = L.load()
    assert lib.toda_conv3x3_transform_weight_batch(None, 0, None) == 0                  # no layers: nothing to do
    assert lib.toda_conv3x3_transform_weight_batch(None, 2, None) == -1 and b"null table" in lib.toda_last_error()
    assert ctypes.sizeof(L.Conv3x3WeightEntry) == 32                                    # the struct of include/toda.h
    table = (L.Conv3x3WeightEntry * 2)()
    for ent, (cout, cin, mode) in zip(table, ((32, 32, 2), (64, 32, 3))):
        ent.w, ent.u, ent.cout, ent.cin, ent.mode = 4096, 4096, cout, cin, mode
    assert lib.toda_conv3x3_transform_weight_batch(L.hptr(table), 2, None) == -1 and b"entry 1" in lib.toda_last_error()
    table[1].mode, table[1].cin = 2, 40                                                 # mode 2 needs both channel counts % 32
    assert lib.toda_conv3x3_transform_weight_batch(L.hptr(table), 2, None) == -1 and b"entry 1" in lib.toda_last_error()
    table[1].u = None
    assert lib.toda_conv3x3_transform_weight_batch(L.hptr(table), 2, None) == -1 and b"null pointer" in lib.toda_last_error()
