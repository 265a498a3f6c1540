"""Host -> device prefetch on a side HIP stream (the role of dataset/data_prefetcher.py:6-106 in the reference's
training loop, train_yolov5.py:458-497): while a step computes, the next batch is already being copied; `next()`
orders the compute stream behind that copy and marks the tensors as used on it."""
import torch

__all__ = ["DataPrefetcher", "TestDataPrefetcher", "DeviceLetterboxPrefetcher", "DeviceLetterboxTestPrefetcher", "DeviceAugmentPrefetcher"]


class _Prefetcher:
    """keys in `tensor_keys` are moved to the device, every other entry of the batch dict is passed through"""
    tensor_keys = ()
    all_keys = ()

    def __init__(self, loader):
        self._it = iter(loader)
        self.stream = torch.cuda.Stream()
        self._staged = None
        self.preload()

    def _stage(self, batch):
        """host batch -> the dict `next()` hands out (runs on the side stream)"""
        return {k: (batch[k].cuda(non_blocking=True) if k in self.tensor_keys else batch[k]) for k in self.all_keys}

    def preload(self):
        batch = next(self._it, None)
        if batch is None:
            self._staged = None
            return
        with torch.cuda.stream(self.stream):
            self._staged = self._stage(batch)

    def next(self):
        current = torch.cuda.current_stream()
        current.wait_stream(self.stream)
        out = self._staged if self._staged is not None else {k: None for k in self.all_keys}
        for k in self.tensor_keys:
            if out[k] is not None:
                out[k].record_stream(current)
        self.preload()
        return out


class DataPrefetcher(_Prefetcher):
    tensor_keys = ('img', 'ann')
    all_keys = ('img', 'ann', 'resize_info', 'img_id')


class TestDataPrefetcher(_Prefetcher):
    tensor_keys = ('img',)
    all_keys = ('img', 'resize_info')


class _DeviceLetterbox(_Prefetcher):
    """for loaders that collate with raw_imgsize_collate_fn / raw_test_collate_fn: the uint8 images and the index tables are
    copied on the side stream and one kernel (hipk.letterbox_batch) writes 'img' there, into a fresh tensor for every batch (a
    consumer may hold batch n while n + 1 is produced).  `next()` returns what DataPrefetcher / TestDataPrefetcher return."""
    raw_keys = ('raw', 'img_off', 'src_hw', 'rows', 'cols')

    def __init__(self, loader, fill_value=128):
        self.fill_value = fill_value
        super().__init__(loader)

    def _stage(self, batch):
        from .. import hipk
        raw, img_off, src_hw, rows, cols = (batch[k].cuda(non_blocking=True) for k in self.raw_keys)
        img = torch.empty(rows.shape[0], 3, rows.shape[1], cols.shape[1], dtype=torch.float32, device=raw.device)
        hipk.letterbox_batch(raw, img_off, src_hw, rows, cols, img, self.fill_value)
        out = {k: (batch[k].cuda(non_blocking=True) if k in self.tensor_keys else batch[k]) for k in self.all_keys if k != 'img'}
        out['img'] = img
        return out


class DeviceLetterboxPrefetcher(_DeviceLetterbox):
    tensor_keys = ('img', 'ann')
    all_keys = ('img', 'ann', 'resize_info', 'img_id')


class DeviceLetterboxTestPrefetcher(_DeviceLetterbox):
    tensor_keys = ('img',)
    all_keys = ('img', 'resize_info')


class DeviceAugmentPrefetcher(_Prefetcher):
    """for loaders that collate with augment_collate_fn: the uint8 images and the plan tables are copied on the side stream and one
    kernel (hipk.augment_batch: mosaic, warp, flips, HSV) writes 'img' there, into a fresh tensor for every batch.  `next()` returns
    what DataPrefetcher returns."""
    tensor_keys = ('img', 'ann')
    all_keys = ('img', 'ann', 'resize_info', 'img_id')
    raw_keys = ('raw', 'tiles', 'canvas_hw', 'minv')

    def __init__(self, loader, fill_value=128):
        self.fill_value = fill_value
        super().__init__(loader)

    def _stage(self, batch):
        from .. import hipk
        raw, tiles, canvas_hw, minv = (batch[k].cuda(non_blocking=True) for k in self.raw_keys)
        gains = batch['hsv_gain'].cuda(non_blocking=True) if batch['hsv_gain'] is not None else None
        H, W = batch['dst_size']
        img = torch.empty(minv.shape[0], 3, H, W, dtype=torch.float32, device=raw.device)
        hipk.augment_batch(raw, tiles, canvas_hw, minv, gains, img, self.fill_value)
        out = {k: (batch[k].cuda(non_blocking=True) if k in self.tensor_keys else batch[k]) for k in self.all_keys if k != 'img'}
        out['img'] = img
        return out
