# The reference's Detection evaluation: eval.py on VOC 2007's test list, Faster-RCNN / ResNet-101 -> mean AP (11-point metric).
# Run from cv_a-fan_amd/ like the reference runs from Detection/; -d names the directory that holds VOCdevkit/, CKPT a checkpoint
# written by train_aug_sat_muti_advt.py (cmd/run_det.sh leaves it there).  Without the data: bash cmd/run_det_eval.sh --synthetic 64
# (random images of VOC's sizes with boxes); further flags are passed on.
DATA=./data
CKPT=${CKPT:-./outputs/ckpt-s1p3g0.5e2_rand_clip-voc2007-resnet101/model-90000.pth}

python -u eval.py -s voc2007 -b resnet101 \
-d ${DATA} \
"$@" \
${CKPT}
