"""ConcatenatedEmbeddingDataset: `{obs_id: {category: [float]*E}}` -> data[N, S*E] fp32.

Counterpart of codae/dataset/concatenated_embedding_dataset.py:9-143 (same constructor,
attributes, `__getitem__ -> (row, idx)` and `.to(device)`), built with whole-array numpy
operations instead of N x S torch.cat calls.  The matrix is what stays resident in HBM and what
the gather kernel reads (codae_batch.data).
"""
import numpy as np
import torch
from torch.utils.data.dataset import Dataset


class ConcatenatedEmbeddingDataset(Dataset):

    def __init__(self, embeddings, used_category, transform=None, keep_incomplete=False, min_present=2):
        """keep_incomplete: keep the observations that have at least `min_present` of the used categories instead of only
        those that have all of them; a category an observation lacks is stored as zeros (in data and in data_per_category),
        `presence` is the uint8 [N, S] table of what is there (codae.tool.SlotPresence takes it) and min / max / scale are taken
        over the present entries only.  The default is the reference's filter, and `presence` is then None."""
        self.embeddings = embeddings
        self.transform = transform
        self.used_category = used_category
        self.nb_used_category = len(used_category)
        self.keep_incomplete = bool(keep_incomplete)
        self.presence = None

        if not self.keep_incomplete:
            # keep observations that have every used category (reference :28-38)
            self.index = [k for k, v in embeddings.items() if all(c in v for c in used_category)]
            self.filtered_embeddings = {k: embeddings[k] for k in self.index}
            self.nb_observation = len(self.index)
            self.embedding_size = len(self.filtered_embeddings[self.index[0]][used_category[0]])

            blocks = [np.asarray([self.filtered_embeddings[k][c] for k in self.index], dtype=np.float32)
                      .reshape(self.nb_observation, self.embedding_size) for c in used_category]
            # raw per-slot matrices stay unscaled (reference :62-63; RankingLoss compares against them)
            self.data_per_category = {n: torch.from_numpy(b.copy()) for n, b in enumerate(blocks)}
            data = torch.from_numpy(np.concatenate(blocks, axis=1))

            # global (max - min) scaling with no shift (reference :69-74)
            self.min = data.min()
            self.max = data.max()
            self.scale = (self.max - self.min).item()
            self.data = data / self.scale
        else:
            if isinstance(min_present, bool) or not isinstance(min_present, int) or not 1 <= min_present <= len(used_category):
                raise ValueError("min_present must be an int in [1, %d], got %r" % (len(used_category), min_present))
            self.index = [k for k, v in embeddings.items() if sum(c in v for c in used_category) >= min_present]
            if not self.index:
                raise ValueError("no observation has %d of the used categories" % min_present)
            self.filtered_embeddings = {k: embeddings[k] for k in self.index}
            self.nb_observation = len(self.index)
            first = self.filtered_embeddings[self.index[0]]
            self.embedding_size = len(first[next(c for c in used_category if c in first)])
            N, E = self.nb_observation, self.embedding_size
            presence = np.zeros((N, len(used_category)), dtype=np.uint8)
            blocks = []
            for n, c in enumerate(used_category):
                block = np.zeros((N, E), dtype=np.float32)
                for r, k in enumerate(self.index):
                    v = self.filtered_embeddings[k].get(c)
                    if v is not None:
                        block[r] = np.asarray(v, dtype=np.float32).reshape(E)
                        presence[r, n] = 1
                blocks.append(block)
            self.presence = presence
            self.data_per_category = {n: torch.from_numpy(b.copy()) for n, b in enumerate(blocks)}
            data = torch.from_numpy(np.concatenate(blocks, axis=1))
            here = torch.from_numpy(np.repeat(presence, E, axis=1).astype(bool))
            # the same global scaling, over what is there: the zeros of an absent slot are no observation of the data's range
            self.min = data[here].min()
            self.max = data[here].max()
            self.scale = (self.max - self.min).item()
            self.data = data / self.scale          # (0 / scale: an absent slot stays exactly 0)

        self.arch = []
        self.io_size = 0
        for name in used_category:
            self.arch.append({"name": name, "lambda": 1, "size": self.embedding_size,
                              "type": "regression", "position": self.io_size})
            self.io_size += self.embedding_size
        self.type_mask = torch.ones((self.io_size))
        self.nb_predictor = self.embedding_size * self.nb_used_category

    def __len__(self):
        return self.nb_observation

    def __getitem__(self, idx):
        if self.transform is not None:
            return self.transform(self.data[idx]), idx
        return self.data[idx], idx

    def to(self, device):
        self.data = self.data.to(device)
        for i in range(len(self.data_per_category)):
            self.data_per_category[i] = self.data_per_category[i].to(device)
