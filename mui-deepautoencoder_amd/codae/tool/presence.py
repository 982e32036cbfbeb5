"""Per-row slot presence: train, evaluate and complete on rows that lack an item in some slots (include/codae_hip.h,
"Slot presence").

A presence table is uint8 [N, S]: table[r][s] == 0 says that dataset row r has no item in slot s.  It is keyed by the DATASET
row, never by the position in a batch.  The rule is selection, not multiplication: what the data matrix holds in an absent slot is
never used by the fused step (it may be NaN) - the gather writes 0 there, the loss and the monitors skip the element, the slot
contrast neither scores the pair nor draws the row as a candidate for that slot.  Nothing renormalises: the loss stays divided by
rows * io, as with LossEmphasis; `counts` gives the monitors' denominators for a caller that wants per-present-element errors.

SlotPresence carries the table, hands it to the HIP engine (DaeEngine.set_slot_presence, HipEmbeddingTrainer(presence=...)) and
gives the drop-in loops the same definition in torch ops: `apply` zeroes the absent slots of a dense batch, `weight` is the 0/1
factor for ReconstructionLoss.loss(weight=...).  (A weight multiplies: with the helpers the absent slots of the data must be
finite - ConcatenatedEmbeddingDataset(keep_incomplete=True) stores zeros there.)  `assign_masks` reorders a Corrupter's mask
assignment so that every run blanks a slot the row actually has.

Not covered: renormalising by present counts, the mixed-variable (abalone) path.  RankingLoss itself ranks complete rows only;
codae.tool.RetrievalMetrics(presence=...) ranks every validation row among the rows that have the slot.
"""
import numpy as np

from ..hip import HipError

MAX_SLOTS = 128


class SlotPresence:
    """SlotPresence(table): table uint8 / bool [N, S] (array or tensor), or None for "every slot of every row is present"."""

    def __init__(self, table=None):
        self._device_tables = {}
        if table is None:
            self.table = None
            return
        t = table.detach().cpu().numpy() if hasattr(table, "detach") else np.asarray(table)
        if t.ndim != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= MAX_SLOTS:
            raise HipError("slot presence: the table must be [n_rows, n_slots] with 1 .. %d slots, got shape %r" % (MAX_SLOTS, tuple(t.shape)))
        if t.dtype.kind not in "bui":
            raise HipError("slot presence: the table must hold booleans or integers, got %s" % t.dtype)
        self.table = np.ascontiguousarray(t != 0).astype(np.uint8)

    def __repr__(self):
        if self.table is None:
            return "SlotPresence(None)"
        return "SlotPresence([%d, %d], %d absent)" % (self.table.shape[0], self.table.shape[1], int((self.table == 0).sum()))

    @property
    def is_default(self):
        """No table, or a table without an absent slot: the engine runs exactly what it runs without one."""
        return self.table is None or bool(self.table.all())

    @property
    def n_rows(self):
        return None if self.table is None else int(self.table.shape[0])

    @property
    def n_slots(self):
        return None if self.table is None else int(self.table.shape[1])

    def to(self, device):
        """The table as a contiguous uint8 tensor on `device` (cached per device); None without a table."""
        import torch
        if self.table is None:
            return None
        device = torch.device(device)
        t = self._device_tables.get(device)
        if t is None:
            t = torch.from_numpy(self.table).to(device).contiguous()
            self._device_tables[device] = t
        return t

    # ---- dense batches (drop-in loops) ---------------------------------------------------------------------------------
    def _rows(self, rows):
        r = rows.detach().cpu().numpy() if hasattr(rows, "detach") else np.asarray(rows)
        r = r.astype(np.int64).reshape(-1)
        if self.table is not None and r.size and (r.min() < 0 or r.max() >= self.table.shape[0]):
            raise HipError("slot presence: dataset rows outside [0, %d)" % self.table.shape[0])
        return r

    def weight(self, rows, E, device=None, dtype=None):
        """float [B, S * E]: 1 on the columns of a present slot of dataset rows `rows`, 0 on an absent one."""
        import torch
        if self.table is None:
            raise HipError("slot presence: weight() needs a table (the number of slots is the table's)")
        if isinstance(E, bool) or int(E) < 1:
            raise HipError("slot presence: E must be a positive int, got %r" % (E,))
        w = np.repeat(self.table[self._rows(rows)], int(E), axis=1)
        return torch.from_numpy(w).to(device=device, dtype=dtype or torch.float32)

    def apply(self, x, rows):
        """x [B, S * E] with the absent slots of dataset rows `rows` set to exactly 0 (a select: a NaN there does not survive)."""
        import torch
        if self.table is None:
            return x
        if x.dim() != 2 or x.shape[1] % self.table.shape[1] != 0 or x.shape[0] != len(self._rows(rows)):
            raise HipError("slot presence: batch shape %s does not fit %d rows of %d slots" % (tuple(x.shape), len(self._rows(rows)), self.table.shape[1]))
        keep = self.weight(rows, x.shape[1] // self.table.shape[1], device=x.device, dtype=torch.bool)
        return torch.where(keep, x, torch.zeros((), dtype=x.dtype, device=x.device))

    def counts(self, rows, mask_ids=None, mask_table=None):
        """(present slots, present-and-blanked slots) summed over dataset rows `rows`, from the tables alone; multiplied by E they
        are the numbers of elements CODAE_S_SQ_FULL and CODAE_S_SQ_PARTIAL add up.  mask_ids [B]: the mask-table row of every
        batch row; mask_table [n_masks, io] 0/1 (whole slots are blanked: column s * E decides slot s).  Without them the second
        count is 0."""
        r = self._rows(rows)
        if self.table is None:
            raise HipError("slot presence: counts() needs a table")
        p = self.table[r] != 0
        full = int(p.sum())
        if mask_ids is None or mask_table is None:
            return full, 0
        ids = mask_ids.detach().cpu().numpy() if hasattr(mask_ids, "detach") else np.asarray(mask_ids)
        mt = mask_table.detach().cpu().numpy() if hasattr(mask_table, "detach") else np.asarray(mask_table)
        S = self.table.shape[1]
        if mt.ndim != 2 or mt.shape[1] % S != 0:
            raise HipError("slot presence: mask table of %r columns does not fit %d slots" % (mt.shape, S))
        blank = mt[ids.astype(np.int64).reshape(-1)][:, ::mt.shape[1] // S] == 0
        if blank.shape != p.shape:
            raise HipError("slot presence: %d mask ids for %d rows" % (blank.shape[0], p.shape[0]))
        return full, int((p & blank).sum())

    # ---- the Corrupter's assignment ------------------------------------------------------------------------------------
    def assign_masks(self, corrupter):
        """int32 [N, nb_run]: every row of corrupter.mask_to_use as its STABLE PARTITION, usable masks first.  A mask is usable
        for a row when every slot it blanks is present in the row and at least one present slot stays visible.  No random numbers
        are drawn, a complete row keeps its order (an all-ones table returns mask_to_use unchanged), and a row without a usable
        mask raises.  Runs [0, usable count of the row) then blank only slots the row has."""
        import torch
        m2u = corrupter.mask_to_use.detach().cpu().numpy().astype(np.int64)
        if self.table is None:
            return torch.from_numpy(m2u.astype(np.int32))
        N, S = self.table.shape
        masks = corrupter.binary_masks.detach().cpu().numpy()
        if m2u.shape[0] != N or masks.shape[1] % S != 0:
            raise HipError("slot presence: corrupter of %d rows / %d columns does not fit a [%d, %d] table" % (m2u.shape[0], masks.shape[1], N, S))
        blanks = masks[:, ::masks.shape[1] // S] == 0                    # [n_masks, S]
        pres = self.table != 0                                           # [N, S]
        b = blanks[m2u]                                                  # [N, nb_run, S]
        usable = ~(b & ~pres[:, None, :]).any(axis=2) & (pres[:, None, :] & ~b).any(axis=2)
        bad = np.nonzero(~usable.any(axis=1))[0]
        if bad.size:
            raise HipError("slot presence: row %d (%d present slots) has no usable mask" % (int(bad[0]), int(pres[bad[0]].sum())))
        order = np.argsort(~usable, axis=1, kind="stable")
        return torch.from_numpy(np.take_along_axis(m2u, order, axis=1).astype(np.int32))
