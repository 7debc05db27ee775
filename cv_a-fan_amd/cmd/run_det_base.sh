# The reference's Detection baseline (sh/voc2007/clean101/080_voc_res101_clean_baseline.sh): train_baseline.py on VOC 2007,
# Faster-RCNN / ResNet-101.  Run from cv_a-fan_amd/; -d names the directory that holds VOCdevkit/.  Without the data: add
# --synthetic 64.
DATA=./data
OUT=./outputs

python -u train_baseline.py -s voc2007 -b resnet101 \
-d ${DATA} \
-o ${OUT} \
--batch_size=8 \
--learning_rate=0.008 \
--step_lr_sizes="[6250, 8750]" \
--num_steps_to_snapshot=1250 \
--num_steps_to_finish=11250 \
--seed 1
