from .train_batch import OccluderBank, TrainBatchMaker, draw_augm_params, draw_meta_mask, draw_occlusions  # noqa: F401
