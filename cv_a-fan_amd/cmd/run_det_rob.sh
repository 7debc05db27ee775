# The reference's Detection robust evaluation: eval_rob_ori.py on VOC 2007's test list, Faster-RCNN / ResNet-101 -> mean AP under a
# 10-step image PGD (eps 2/255, step 0.5/255) on the sum of the four training losses.  Run from cv_a-fan_amd/ like the reference runs
# from Detection/; -d names the directory that holds VOCdevkit/, CKPT a checkpoint written by train_aug_final.py or
# train_aug_sat_muti_advt.py.  Without the data: bash cmd/run_det_rob.sh --synthetic 64; further flags are passed on.
DATA=./data
CKPT=${CKPT:-./outputs/ckpt-s1p3g0.5e2_rand_clip-voc2007-resnet101/model-90000.pth}

python -u eval_rob_ori.py -s voc2007 -b resnet101 \
--steps 10 --gamma 0.5 --eps 2 --clip \
-d ${DATA} \
"$@" \
${CKPT}
