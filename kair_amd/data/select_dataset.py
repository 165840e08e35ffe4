"""Dataset factory (mirror of /root/reference/data/select_dataset.py:12-100) for the datasets that
feed the kair_amd hot path: 'dncnn' (DatasetDnCNN, config 1), 'fdncnn' / 'drunet' (DatasetFDnCNN: the noisy image
plus its noise-level map, train_fdncnn.json and train_drunet.json), 'ffdnet' (DatasetFFDNet: the noisy image and its
noise level as a second input "C"), 'sr' (DatasetSR, configs 2/4/5),
'usrnet' (DatasetUSRNet, config 3), 'jpeg' (DatasetJPEG, the JPEG artifact-reduction SwinIR of
train_swinir_car_jpeg.json) and 'blindsr' (DatasetBlindSR, the BSRGAN degradation of
train_bsrgan_x4_psnr.json and train_swinir_sr_realworld_x4_psnr.json) and 'srmd' (DatasetSRMD: the degraded LR image
followed by its degradation map, train_srmd.json).
Other dataset types are off the path and raise NotImplementedError naming the type."""


def define_Dataset(dataset_opt):
    t = dataset_opt["dataset_type"].lower()
    if t in ("dncnn", "denoising"):
        from .dataset_dncnn import DatasetDnCNN as D
    elif t in ("fdncnn", "drunet"):
        from .dataset_fdncnn import DatasetFDnCNN as D
    elif t == "ffdnet":
        from .dataset_ffdnet import DatasetFFDNet as D
    elif t in ("sr", "super-resolution"):
        from .dataset_sr import DatasetSR as D
    elif t == "usrnet":
        from .dataset_usrnet import DatasetUSRNet as D
    elif t == "jpeg":
        from .dataset_jpeg import DatasetJPEG as D
    elif t in ("blindsr", "bsrnet", "bsrgan"):
        from .dataset_blindsr import DatasetBlindSR as D
    elif t == "srmd":
        from .dataset_srmd import DatasetSRMD as D
    elif t == "dpsr":   # the noisy bicubic LR image followed by its noise-level channel (train_dpsr.json)
        from .dataset_dpsr import DatasetDPSR as D
    else:
        raise NotImplementedError(f"Dataset [{t}] is not on the kair_amd path (dncnn, fdncnn, drunet, ffdnet, sr, usrnet, jpeg, "
                                  "blindsr, srmd, dpsr).")
    return D(dataset_opt)
