# The reference README's Detection recipe: train_aug_final.py on VOC 2007, Faster-RCNN / ResNet-101, batch 8 — feature PGD behind
# backbone layer 2 with sample points 3 and 4 mixed, ROI-feature PGD under the two proposal losses at weight 0.3 — then eval.py on
# the last checkpoint.  Run from cv_a-fan_amd/ like the reference runs from Detection/; -d names the directory that holds
# VOCdevkit/.  Without the data: add --synthetic 64 to both commands.
DATA=./data
OUT=./outputs

python -u train_aug_final.py -s voc2007 -b resnet101 \
-d ${DATA} \
-o ${OUT} \
--batch_size=8 \
--learning_rate=0.008 \
--step_lr_sizes="[6250, 8750]" \
--num_steps_to_snapshot=1250 \
--num_steps_to_finish=11250 \
--mix_layer 0011 \
--pertub_idx_se 2 \
--gamma_se 1.0 \
--gamma_sd 0.1 \
--sd_adv_loss_weight 0.3 \
--only_roi_sd \
--seed 1 \
&& python -u eval.py -s voc2007 -b resnet101 -d ${DATA} \
${OUT}/ckpt-s1se_2_sd_roi_g1.0e2_MIX0011-voc2007-resnet101/model-11250.pth
