# The reference's Detection training run: train_aug_sat_muti_advt.py on VOC 2007, Faster-RCNN / ResNet-101, loss setting 1
# (the multi-layer SAT loss alone).  Run from cv_a-fan_amd/ like the reference runs from Detection/; -d names the directory that
# holds VOCdevkit/.  Without the data: add --synthetic 64 (random images of VOC's sizes with boxes).
DATA=./data
OUT=./outputs

python -u train_aug_sat_muti_advt.py -s voc2007 -b resnet101 \
-d ${DATA} \
-o ${OUT} \
--loss_settings 1 \
--randinit --clip \
--seed 1
