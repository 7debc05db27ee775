# The reference's Detection layer-wise SAT evaluation: eval_sat_layers.py on VOC 2007's test list, Faster-RCNN / ResNet-101 -> mean AP
# when the feature map behind backbone layer --pertub_idx is replaced by sample point --sat_layer (0 clean .. 4 adversarial) of its
# 10-step feature PGD (eps 2/255, step 0.5/255); --mix re-normalises the point onto the clean map's channel statistics.  --table fills
# all ten (sat_layer, mix) settings from one attack per image.  Run from cv_a-fan_amd/ like the reference runs from Detection/; -d
# names the directory that holds VOCdevkit/, CKPT a checkpoint written by train_aug_final.py or train_aug_sat_muti_advt.py.
# Without the data: bash cmd/run_det_sat.sh --synthetic 64; further flags are passed on.
DATA=./data
CKPT=${CKPT:-./outputs/ckpt-s1p3g0.5e2_rand_clip-voc2007-resnet101/model-90000.pth}

python -u eval_sat_layers.py -s voc2007 -b resnet101 \
--steps 10 --gamma 0.5 --eps 2 --clip \
--pertub_idx 3 --sat_layer 1 --table \
-d ${DATA} \
"$@" \
${CKPT}
