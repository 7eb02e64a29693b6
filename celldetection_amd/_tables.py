"""Host side of the keyed device tables (``csrc/label_table.h``): the first capacity of a table and the loop that repeats a
pass with twice the capacity until every key found a slot."""

__all__ = ['default_capacity', 'check_capacity', 'grow_until_it_fits']


def default_capacity(pixels, pixels_per_slot):
    """4096 slots, doubled while below one slot per ``pixels_per_slot`` pixels and below 2 ** 21."""
    cap = 1 << 12
    while cap < pixels // pixels_per_slot and cap < (1 << 21):
        cap <<= 1
    return cap


def check_capacity(cap):
    if cap < 2 or cap & (cap - 1):
        raise ValueError('table_capacity must be a power of two')


def grow_until_it_fits(cap, attempt):
    """``attempt(cap)`` allocates a workspace, runs the pass and returns ``(workspace, overflow, entries)``; ``overflow`` counts
    the inserts that found no slot within their probe limit.  -> ``(workspace, cap, grown, entries)`` of the first attempt
    without overflow, ``grown`` the number of doublings.  The workspace of a failed attempt is dropped before the next one."""
    grown = 0
    while True:
        ws, overflow, entries = attempt(cap)
        if overflow == 0:
            return ws, cap, grown, entries
        del ws
        cap *= 2
        grown += 1
