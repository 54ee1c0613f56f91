from .train_batch import TrainBatchMaker, draw_augm_params, draw_meta_mask  # noqa: F401
