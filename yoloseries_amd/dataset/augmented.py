"""AugmentedDataset: a detection dataset whose items are augmentation plans (utils/augment.py) instead of augmented pixels.  The
role of YOLODataset.__getitem__ with enable_data_aug (dataset/CommonDataloader.py:387-429 of the reference): the draws and the label
arithmetic happen here, in the loader's workers; the pixels are produced on the GPU from the raw images the item carries."""
import random

import numpy as np
import torch

from ..utils import augment as A

__all__ = ['AugmentedDataset']


class AugmentedDataset:
    """base: any dataset yielding (image (h, w, 3) uint8, {'bboxes': (n, 4) xyxy, 'classes': n}, id).
    __getitem__ -> ([raw uint8 images of the plan: 1 or 4], plan, {'bboxes', 'classes'} in the output frame, id); after
    close_data_aug() the base's plain item.  The plan of item i depends on (seed, the worker's seed, the order of requests)."""

    def __init__(self, base, input_dim, aug_hyp, seed=0):
        self.base, self.input_dim = base, [int(input_dim[0]), int(input_dim[1])]
        self.hyp = A.check_aug_hyp(aug_hyp)
        self.seed = int(seed or 0)
        self.enable_data_aug = True
        self._rng = self._np_rng = None
        self._rng_key = None

    def __len__(self):
        return len(self.base)

    def close_data_aug(self):
        """from now on items are the base's, un-augmented (the last no_data_aug_epoch epochs of a run).  Workers that are already
        running hold their own copy of the dataset: rebuild the loader's iterator (the drivers start one per epoch)."""
        self.enable_data_aug = False

    def seed_worker(self, worker_seed):
        """the host RNGs of this process: Python's and NumPy's, from the dataset's seed and the worker's"""
        self._rng_key = worker_seed
        self._rng = random.Random(f"augment/{self.seed}/{worker_seed}")
        self._np_rng = np.random.RandomState(self._rng.getrandbits(32))

    def _rngs(self):
        info = torch.utils.data.get_worker_info()
        if info is not None and info.seed != self._rng_key:          # a fresh worker (a new epoch) brings a new seed
            self.seed_worker(info.seed)
        elif self._rng is None:
            self.seed_worker(0)
        return self._rng, self._np_rng

    def __getitem__(self, ix):
        if not self.enable_data_aug:
            return self.base[ix]
        rng, np_rng = self._rngs()
        cache = {}

        def item(i):
            if i not in cache:
                cache[i] = self.base[i]
            return cache[i]

        for _ in range(A.MAX_TRIES):                                 # an item that lost all its boxes is drawn again
            plan = A.draw_plan(ix, len(self.base), lambda i: item(i)[0].shape[:2], self.input_dim, self.hyp, rng, np_rng)
            anns = [{'bboxes': np.asarray(item(i)[1]['bboxes']), 'classes': np.asarray(item(i)[1]['classes'])} for i in plan['indices']]
            boxes, classes = A.plan_labels(plan, anns)
            if len(classes) > 0:
                break
        return [item(i)[0] for i in plan['indices']], plan, {'bboxes': boxes, 'classes': classes}, item(ix)[2]
