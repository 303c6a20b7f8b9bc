"""A plain-Python model of "retune with a mask" (bk_retune_*), sharing no text with the library: the verdict of every
entry in the public structs' terms, all-or-nothing per unit, the status pair, the count of refused units and the fields a
retune may not change.  tests/test_retune_cpu.py checks it against hand-written cases; tests/test_gpu_retune.py uses it
as the expected status side of the kernel.

A group row is the 7-tuple of RANDOM_AGENTS_DTYPE ``(n_agents, tick_lo, tick_hi, vol_lo, vol_hi, tick_size,
activity_rate)``; a member row is a dict of AGENT_DESC_DTYPE's fields.  The model's "table" is the list of rows in force,
``table[unit][entry]``: after a retune an applied unit holds the new rows, a refused or unmasked unit its old ones."""
import math

OK, NOT_TICK_MULTIPLE, INVALID = 0, 1, 5  # bk_status
RANDOM, NOISE, MOMENTUM = 0, 1, 2        # bk_agent_type
U32_MAX = 0xFFFFFFFF


def group_verdict(row, book_tick: int, installed_n: int) -> int:
    """The status of one RandomAgents group against the install's checks, then against the installed ``n_agents``."""
    n, tick_lo, tick_hi, vol_lo, vol_hi, tick_size, _rate = row
    if tick_hi <= tick_lo or vol_hi <= vol_lo:
        return INVALID  # an empty range
    if tick_size % book_tick:
        return NOT_TICK_MULTIPLE
    if tick_lo == 0 or (tick_hi - 1) * tick_size >= U32_MAX:
        return INVALID  # a price outside (0, u32::MAX)
    return OK if n == installed_n else INVALID


def member_verdict(row: dict, book_tick: int, installed: dict) -> int:
    """The same for one member; ``installed`` holds the installed ``type``, ``n_agents`` and ``agent_id_start``."""
    ts = row["tick_size"]
    if ts == 0 or ts % book_tick:
        return NOT_TICK_MULTIPLE
    kind = row["type"]
    if kind == RANDOM:
        if row["tick_hi"] <= row["tick_lo"] or row["vol_hi"] <= row["vol_lo"] or row["tick_lo"] == 0:
            return INVALID
        if (row["tick_hi"] - 1) * ts >= U32_MAX:
            return INVALID
    elif kind in (NOISE, MOMENTUM):
        if row["n_agents"] > 0xFFFF:
            return INVALID
        sigma, mu = row["price_dist_sigma"], row["price_dist_mu"]
        if math.isnan(sigma) or math.isinf(sigma) or sigma < 0 or math.isnan(mu) or math.isinf(mu):
            return INVALID
    else:
        return INVALID
    same = all(row[k] == installed[k] for k in ("type", "n_agents", "agent_id_start"))
    return OK if same else INVALID


def retune(table, rows, mask, verdict_of):
    """``table`` / ``rows``: ``[unit][entry]``; ``mask``: per unit or None (every unit); ``verdict_of(unit, entry, row)``:
    the entry's status.  Returns ``(new_table, status, n_refused)`` with ``status[unit] = (code, first failing entry)``."""
    out, status, refused = [], [], 0
    for u, old in enumerate(table):
        if mask is not None and not mask[u]:
            out.append(list(old))
            status.append((OK, 0))
            continue
        bad = [(verdict_of(u, j, r), j) for j, r in enumerate(rows[u])]
        bad = [(c, j) for c, j in bad if c != OK]
        if bad:
            out.append(list(old))
            status.append(bad[0])
            refused += 1
        else:
            out.append(list(rows[u]))
            status.append((OK, 0))
    return out, status, refused


def retune_groups(table, rows, mask, book_ticks, assets=None):
    """Groups: ``book_ticks[asset]`` is the asset's tick, ``assets[entry]`` the installed asset (None: all 0); the
    installed ``n_agents`` is the table's own."""
    def verdict(u, j, r):
        return group_verdict(r, book_ticks[assets[j] if assets else 0], table[u][j][0])
    return retune(table, rows, mask, verdict)


def retune_members(table, rows, mask, book_ticks, assets=None):
    def verdict(u, j, r):
        return member_verdict(r, book_ticks[assets[j] if assets else 0], table[u][j])
    return retune(table, rows, mask, verdict)
