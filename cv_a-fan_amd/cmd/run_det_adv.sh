# The reference's Detection PGD training (train_baseline_advtrain.py) on VOC 2007, Faster-RCNN / ResNet-101: one sign-PGD step of
# 0.5/255 inside the 2/255 ball from a random start on every batch, then the SGD step on the adversarial images.  Run from
# cv_a-fan_amd/; -d names the directory that holds VOCdevkit/.  Without the data: add --synthetic 64.  The start is drawn on the
# device (the default of --noise); --noise host makes a run resumed with -r repeat the uninterrupted run's draws.
DATA=./data
OUT=./outputs

python -u train_baseline_advtrain.py -s voc2007 -b resnet101 \
-d ${DATA} \
-o ${OUT} \
--steps 1 \
--gamma 0.5 \
--eps 2 \
--randinit \
--clip \
--batch_size=8 \
--learning_rate=0.008 \
--step_lr_sizes="[6250, 8750]" \
--num_steps_to_snapshot=1250 \
--num_steps_to_finish=11250 \
--seed 1
