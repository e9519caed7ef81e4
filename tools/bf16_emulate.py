"""CPU emulation of the bf16 inference mode (engine precision="bf16"), to calibrate the network-level bounds of
tests/test_gpu_bf16_predict.py.  Runs the NumPy oracle's ResNet50 forward (oracle/dense.py) twice on the same panel, with its
conv2d replaced by a torch CPU convolution:
  fp32  operands as they are, fp32 accumulation;
  bf16  both operands of every conv rounded to bf16 (round to nearest even) first, fp32 accumulation -- the arithmetic of
        csrc/conv_bf16.hip (the 3-channel stem stays fp32, as in the engine).
and reports the three quantities the GPU test bounds: relative Frobenius error of the feature map F, max |diff| of the RPN
sigmoid outputs, max |diff| of the classifier softmax on the same RoIs (those the fp32 pass proposes).
usage: python tools/bf16_emulate.py [img_size=600] [n_rois=300] [seed=3]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rock-art-radnet_amd")]
import torch  # noqa: E402

from faster_rcnn.config import Config  # noqa: E402
from oracle import dense, glue  # noqa: E402
from radnet_hip import synth  # noqa: E402

MODE = ["fp32"]


def conv2d_torch(x, w, b, stride=1, pad=(0, 0, 0, 0)):
    kh, kw, C, Co = w.shape
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).permute(3, 2, 0, 1)
    if MODE[0] == "bf16" and C % 8 == 0:
        xt = xt.to(torch.bfloat16).to(torch.float32)
        wt = wt.to(torch.bfloat16).to(torch.float32)
    pt, pl, pb, pr = pad
    xt = torch.nn.functional.pad(xt, (pl, pr, pt, pb))
    y = torch.nn.functional.conv2d(xt, wt, None if b is None else torch.from_numpy(np.asarray(b, np.float32)), stride=stride)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def run(P, x, rois, C):
    F = dense.base_forward(P, x)
    pc, pr, _ = dense.rpn_forward(P, F)
    if rois is None:
        fh, fw = F.shape[1], F.shape[2]
        R = glue.rpn_to_roi(pc.reshape(1, fh, fw, -1), pr.reshape(1, fh, fw, -1), C, True, C.n_rois_emulate, 0.7)
        rois = R.astype(np.float32).copy()
        rois[:, 2] -= rois[:, 0]
        rois[:, 3] -= rois[:, 1]
    hc, _, _ = dense.head_forward(P, F, rois)
    return F, pc, hc, rois


def main():
    img_size = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    n_rois = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dense.conv2d = conv2d_torch
    C = Config()
    C.n_rois_emulate = n_rois
    P = synth.synthetic_weights(seed=seed)
    img = synth.synthetic_panel(seed, img_size, img_size)
    x = dense.preprocess_caffe_bgr(img)
    MODE[0] = "fp32"
    F32, p32, c32, rois = run(P, x, None, C)
    MODE[0] = "bf16"
    F16, p16, c16, _ = run(P, x, rois, C)
    relF = float(np.linalg.norm((F16 - F32).astype(np.float64)) / np.linalg.norm(F32.astype(np.float64)))
    drpn = float(np.abs(p16.astype(np.float64) - p32).max())
    dcls = float(np.abs(c16.astype(np.float64) - c32).max())
    print("img_size %d, %d RoIs, weights seed %d" % (img_size, len(rois), seed))
    print("feature map F   relative Frobenius error  %.3e" % relF)
    print("RPN sigmoid     max |bf16 - fp32|         %.3e" % drpn)
    print("classifier      max |bf16 - fp32| softmax %.3e" % dcls)


if __name__ == "__main__":
    main()
